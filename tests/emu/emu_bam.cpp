// TEST INFRASTRUCTURE: CPU twin of the unaligned BAM entry points of atropos_amd/csrc/bam_kernels.hip, built from the
// same per-record and per-tile source (bam_core.hpp) with -DATR_HOST_EMU.  One loop iteration here = one wave (tile of
// the speculative pass), one step of the serial pass, or one thread (tile of the table, record of the decode) of the
// kernels; the prefix sum is a running sum.  The workspace holds what the kernels keep there, in the same layout.
#include <stdint.h>
#include <string.h>
#include <limits.h>

#include "emu_abi.hpp"
#include "bam_core.hpp"

using namespace atr;

namespace {

struct Placed {
    uint32_t entry, base;
};

size_t up(size_t x) { return (x + 255) & ~(size_t)255; }
long long blocks(long long n, long long per) { return (n + per - 1) / per; }

void report(int64_t *result, long long ordinal, int kind) {
    const long long word = ordinal * 8 + kind;
    if (word < result[1]) result[1] = word;
}

}  // namespace

extern "C" {

int emu_bam_header(const uint8_t *buf, int64_t n_bytes, int64_t *header_bytes, int32_t *n_ref) {
    if (n_bytes < 0 || (n_bytes && !buf) || !header_bytes || !n_ref) return ATR_ERR_INVALID;
    long long len = 0;
    int refs = 0;
    const int rc = bam_header_parse(buf, n_bytes, &len, &refs);
    if (rc < 0) return ATR_ERR_INVALID;
    if (rc > 0) return ATR_BAM_NEED_MORE;
    *header_bytes = len;
    *n_ref = refs;
    return ATR_OK;
}
EMU_TWIN(bam_header);

int64_t emu_bam_walk_workspace(int64_t n_bytes, int64_t tile_bytes) {
    if (n_bytes < 0 || tile_bytes < ATR_BAM_MIN_TILE || tile_bytes > ATR_BAM_MAX_TILE) return ATR_ERR_INVALID;
    const long long ntiles = blocks(n_bytes, tile_bytes);
    return (int64_t)(up((size_t)ntiles * sizeof(BamTile)) + up((size_t)ntiles * sizeof(Placed)) + 256);
}
EMU_TWIN(bam_walk_workspace);

int emu_bam_walk(const uint8_t *bam, int64_t n_bytes, int64_t entry, int32_t n_ref, int final, int64_t tile_bytes, int64_t max_block,
                 uint32_t *starts, int64_t starts_capacity, int64_t *result, void *workspace, int64_t workspace_bytes, void *) {
    if (n_bytes < 0 || entry < 0 || entry > n_bytes || n_ref < 0 || tile_bytes < ATR_BAM_MIN_TILE || tile_bytes > ATR_BAM_MAX_TILE ||
        max_block < 32 || max_block > INT_MAX || starts_capacity < 0)
        return ATR_ERR_INVALID;
    if (n_bytes >= (int64_t)0xFFFFFFF0ll) return ATR_ERR_UNSUPPORTED;
    if (!result || (n_bytes && (!bam || !workspace)) || (starts_capacity && !starts) ||
        workspace_bytes < emu_bam_walk_workspace(n_bytes, tile_bytes))
        return ATR_ERR_INVALID;
    const long long n = n_bytes, ntiles = blocks(n, tile_bytes);
    BamTile *tiles = (BamTile *)workspace;
    Placed *placed = (Placed *)((char *)workspace + up((size_t)ntiles * sizeof(BamTile)));
    for (long long t = 0; t < ntiles; ++t) {                  // bam_spec_kernel: the lowest candidate that passes
        const long long tile_end = (t + 1) * tile_bytes;
        const long long lo = t * tile_bytes > entry ? t * tile_bytes : entry;
        const long long hi = tile_end < n - (BAM_FIXED - 1) ? tile_end : n - (BAM_FIXED - 1);
        long long guess = -1;
        for (long long c = lo; c < hi && guess < 0; ++c)
            if (bam_plausible_chain(bam, n, c, n_ref, max_block)) guess = c;
        const BamTile none = {BAM_NONE, 0u, 0u, (uint32_t)BAM_PARTIAL};
        tiles[t] = guess >= 0 ? bam_tile_walk(bam, n, guess, tile_end, max_block) : none;
    }
    BamChain chain = {entry, BAM_OK, 0ull, 0ull};             // bam_resolve_kernel
    for (long long t = 0; t < ntiles; ++t)
        bam_resolve_tile(bam, n, max_block, (t + 1) * tile_bytes, tiles[t], chain, placed[t].entry, placed[t].base);
    long long words[4];
    bam_chain_result(chain, n, final, words);
    for (int k = 0; k < 4; ++k) result[k] = words[k];
    for (long long t = 0; t < ntiles; ++t) {                  // bam_starts_kernel
        if (placed[t].entry == BAM_NONE) continue;
        const long long end = (t + 1) * tile_bytes < words[1] ? (t + 1) * tile_bytes : words[1];
        long long at = placed[t].entry, slot = placed[t].base;
        while (at < end && at + 4 <= n) {
            if (slot < starts_capacity) starts[slot] = (uint32_t)at;
            ++slot;
            const long long bs = bam_i32(bam + at);
            if (bs < 32) break;
            at += 4 + bs;
        }
    }
    return ATR_OK;
}
EMU_TWIN(bam_walk);

size_t emu_bam_to_fastq_work_bytes(int64_t n) { return n < 0 ? 0 : 16; }
EMU_TWIN(bam_to_fastq_work_bytes);

int emu_bam_to_fastq(const uint8_t *bam, int64_t n_bytes, const uint32_t *starts, int64_t n, int paired, int64_t *offsets,
                     int64_t *result, void *work, uint8_t *out, void *) {
    if (n_bytes < 0 || n < 0 || n > n_bytes) return ATR_ERR_INVALID;
    if (n_bytes >= (int64_t)0x7FFFFFF0ll) return ATR_ERR_UNSUPPORTED;
    if (!offsets || !result) return ATR_ERR_INVALID;
    const long long used = paired ? (n & ~(int64_t)1) : n;
    if (used && (!bam || !starts || !work)) return ATR_ERR_INVALID;
    if (!out) {
        result[0] = 0;
        result[1] = LLONG_MAX;
        result[2] = used;
        offsets[0] = 0;
    }
    long long run = 0;
    for (long long j = 0; j < used; ++j) {
        long long src = j;
        int pair_error = 0;
        if (paired) src = bam_pair_source(bam, starts, j, pair_error);
        const BamFields f = bam_fields(bam, starts[src]);
        if (!out) {
            if (pair_error && !(j & 1)) report(result, j, pair_error);
            const int error = bam_record_check(f);
            if (error) report(result, src, error);
            offsets[j] = run;
            run += (long long)bam_text_bytes(f);
        } else {
            const int error = bam_format_record(out + offsets[j], bam, f, 0, 1);
            if (error) report(result, src, error);
        }
    }
    if (!out) {
        offsets[used] = run;
        result[0] = run;
    }
    return ATR_OK;
}
EMU_TWIN(bam_to_fastq);

}  // extern "C"
