// bam_kernels.hip -- unaligned BAM input on the device: the record walk over a chunk of inflated BAM bytes and the
// decode of its records into FASTQ text (see include/atropos_hip.h, "unaligned BAM input"; the per-record and
// per-tile code is bam_core.hpp).
//
// The walk, three launches and no word to the host in between:
//   1. bam_spec_kernel     a wave per tile: its lanes test 64 candidate offsets at a time for a plausible record and
//                          the record chain behind it; the wave walks the tile from the first one that passes;
//   2. bam_resolve_kernel  ONE wave follows the true chain from tile to tile.  64 tiles' results are staged in LDS by
//                          all lanes, lane 0 passes them (a compare per tile whose guess was right, a second walk of
//                          the tile where it was not) and leaves every tile's true first start and the number of
//                          records in front of it;
//   3. bam_starts_kernel   a thread per tile writes the tile's record starts to their place in the table.
// The decode: a thread per output record sizes it, an exclusive prefix sum places it, 16 lanes per record write it.
// The only atomic is the minimum of the decode's error word.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "atropos_hip.h"
#include "bam_core.hpp"

#include "launch_util.hpp"
#include "scan_kernels.hpp"

namespace atr {
namespace {

constexpr int BAM_EMIT_LANES = 16;

// ------------------------------------------------------------------------- the walk
__global__ __launch_bounds__(256) void bam_spec_kernel(const uint8_t *__restrict__ bytes, long long n, long long entry, int n_ref,
                                                       long long tile_bytes, long long cap, long long ntiles,
                                                       BamTile *__restrict__ tiles) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);          // wave-uniform
    if (t >= ntiles) return;
    const long long tile_end = (t + 1) * tile_bytes;
    const long long lo = max(t * tile_bytes, entry), hi = min(tile_end, n - (BAM_FIXED - 1));   // candidates: [lo, hi)
    long long guess = -1;
    for (long long c0 = lo; c0 < hi && guess < 0; c0 += 64) {
        const long long c = c0 + lane;
        const bool ok = c < hi && bam_plausible_chain(bytes, n, c, n_ref, cap);
        const u64 mask = __ballot(ok);
        if (mask) guess = c0 + (__ffsll((long long)mask) - 1);
    }
    BamTile tile = {BAM_NONE, 0u, 0u, (uint32_t)BAM_PARTIAL};
    if (guess >= 0) tile = bam_tile_walk(bytes, n, guess, tile_end, cap);        // (every lane the same walk)
    if (lane == 0) tiles[t] = tile;
}

__global__ __launch_bounds__(64) void bam_resolve_kernel(const uint8_t *__restrict__ bytes, long long n, long long entry, int final,
                                                         long long tile_bytes, long long cap, long long ntiles,
                                                         const BamTile *__restrict__ tiles, uint2 *__restrict__ placed,
                                                         long long *__restrict__ result) {
    __shared__ BamTile s_tile[64];
    __shared__ uint2 s_placed[64];
    const int lane = threadIdx.x;
    BamChain chain = {entry, BAM_OK, 0ull, 0ull};
    for (long long t0 = 0; t0 < ntiles; t0 += 64) {
        const int here = (int)min<long long>(64, ntiles - t0);
        if (lane < here) s_tile[lane] = tiles[t0 + lane];
        __syncthreads();
        if (lane == 0) {
            for (int k = 0; k < here; ++k) {
                uint32_t first, base;
                bam_resolve_tile(bytes, n, cap, (t0 + k + 1) * tile_bytes, s_tile[k], chain, first, base);
                s_placed[k] = make_uint2(first, base);
            }
        }
        __syncthreads();
        if (lane < here) placed[t0 + lane] = s_placed[lane];
    }
    if (lane == 0) bam_chain_result(chain, n, final, result);
}

__global__ __launch_bounds__(256) void bam_starts_kernel(const uint8_t *__restrict__ bytes, long long n, long long tile_bytes,
                                                         long long ntiles, const uint2 *__restrict__ placed,
                                                         const long long *__restrict__ result, uint32_t *__restrict__ starts,
                                                         long long capacity) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= ntiles) return;
    const uint2 mine = placed[t];
    if (mine.x == BAM_NONE) return;
    const long long end = min((t + 1) * tile_bytes, result[1]);                  // result[1]: the end of the last whole record
    long long at = mine.x, slot = mine.y;
    while (at < end && at + 4 <= n) {                                            // (every record in front of `end` is whole)
        if (slot < capacity) starts[slot] = (uint32_t)at;
        ++slot;
        const long long bs = bam_i32(bytes + at);
        if (bs < 32) break;                                                      // (never: the chain's records passed bam_step)
        at += 4 + bs;
    }
}

__global__ void bam_total_kernel(const long long *offsets, long long used, long long *result) { result[0] = offsets[used]; }

__global__ void bam_result_kernel(long long *result, long long *offsets, long long used) {
    result[0] = 0;
    result[1] = LLONG_MAX;
    result[2] = used;
    if (offsets) offsets[0] = 0;
}

// ------------------------------------------------------------------------- decode
__device__ __forceinline__ void bam_report(long long *result, long long ordinal, int kind) {
    atomicMin((u64 *)result + 1, (u64)ordinal * 8ull + (u64)kind);
}

__global__ __launch_bounds__(256) void bam_sizes_kernel(const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ starts,
                                                        long long used, int paired, u64 *__restrict__ sizes,
                                                        long long *__restrict__ result) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= used) return;
    long long src = j;
    if (paired) {
        int error;
        src = bam_pair_source(bytes, starts, j, error);
        if (error && !(j & 1)) bam_report(result, j, error);
    }
    const BamFields f = bam_fields(bytes, starts[src]);
    const int error = bam_record_check(f);
    if (error) bam_report(result, src, error);
    sizes[j] = bam_text_bytes(f);
}

__global__ __launch_bounds__(256) void bam_emit_kernel(const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ starts,
                                                       long long used, int paired, const long long *__restrict__ offsets,
                                                       uint8_t *__restrict__ out, long long *__restrict__ result) {
    const long long j = ((long long)blockIdx.x * 256 + threadIdx.x) / BAM_EMIT_LANES;
    const int part = threadIdx.x % BAM_EMIT_LANES;
    if (j >= used) return;
    long long src = j;
    if (paired) {
        int ignored;
        src = bam_pair_source(bytes, starts, j, ignored);
    }
    const int error = bam_format_record(out + offsets[j], bytes, bam_fields(bytes, starts[src]), part, BAM_EMIT_LANES);
    if (error) bam_report(result, src, error);
}

// work layout of the walk: [BamTile x ntiles][uint2 x ntiles]
struct WalkWork {
    long long ntiles;
    BamTile *tiles;
    uint2 *placed;
    size_t bytes;
};

WalkWork walk_work(void *work, long long n_bytes, long long tile_bytes) {
    WalkWork w;
    Workspace ws(work);
    w.ntiles = blocks(n_bytes, tile_bytes);
    w.tiles = ws.take<BamTile>((size_t)w.ntiles);
    w.placed = ws.take<uint2>((size_t)w.ntiles);
    w.bytes = ws.bytes();
    return w;
}

}  // namespace
}  // namespace atr

using namespace atr;

extern "C" {

int atr_bam_header(const uint8_t *buf, int64_t n_bytes, int64_t *header_bytes, int32_t *n_ref) {
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

int64_t atr_bam_walk_workspace(int64_t n_bytes, int64_t tile_bytes) {
    if (n_bytes < 0 || tile_bytes < ATR_BAM_MIN_TILE || tile_bytes > ATR_BAM_MAX_TILE) return ATR_ERR_INVALID;
    return (int64_t)walk_work(nullptr, n_bytes, tile_bytes).bytes;
}

int atr_bam_walk(const uint8_t *d_bam, int64_t n_bytes, int64_t entry, int32_t n_ref, int final, int64_t tile_bytes,
                 int64_t max_block, uint32_t *d_starts, int64_t starts_capacity, int64_t *d_result, void *d_workspace,
                 int64_t workspace_bytes, void *stream) {
    if (n_bytes < 0 || entry < 0 || entry > n_bytes || n_ref < 0 || tile_bytes < ATR_BAM_MIN_TILE || tile_bytes > ATR_BAM_MAX_TILE ||
        max_block < 32 || max_block > INT_MAX || starts_capacity < 0)
        return ATR_ERR_INVALID;
    if (n_bytes >= (int64_t)0xFFFFFFF0ll) return ATR_ERR_UNSUPPORTED;
    if (!d_result || (n_bytes && (!d_bam || !d_workspace)) || (starts_capacity && !d_starts) || ((uintptr_t)d_bam & 15) ||
        workspace_bytes < atr_bam_walk_workspace(n_bytes, tile_bytes))
        return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const WalkWork w = walk_work(d_workspace, n_bytes, tile_bytes);
    const long long ntiles = w.ntiles;
    BamTile *tiles = w.tiles;
    uint2 *placed = w.placed;
    if (ntiles)
        hipLaunchKernelGGL(bam_spec_kernel, dim3((unsigned)blocks(ntiles, 4)), dim3(256), 0, st, d_bam, (long long)n_bytes,
                           (long long)entry, (int)n_ref, (long long)tile_bytes, (long long)max_block, ntiles, tiles);
    hipLaunchKernelGGL(bam_resolve_kernel, dim3(1), dim3(64), 0, st, d_bam, (long long)n_bytes, (long long)entry, final,
                       (long long)tile_bytes, (long long)max_block, ntiles, (const BamTile *)tiles, placed, (long long *)d_result);
    if (ntiles)
        hipLaunchKernelGGL(bam_starts_kernel, dim3(grid256(ntiles)), dim3(256), 0, st, d_bam, (long long)n_bytes,
                           (long long)tile_bytes, ntiles, (const uint2 *)placed, (const long long *)d_result, d_starts,
                           (long long)starts_capacity);
    return launched("bam walk launch");
}

// work layout: scan_work of 64-bit sizes, a spare word behind the sums
size_t atr_bam_to_fastq_work_bytes(int64_t n) { return n < 0 ? 0 : scan_work_bytes<u64>(n, 1); }

int atr_bam_to_fastq(const uint8_t *d_bam, int64_t n_bytes, const uint32_t *d_starts, int64_t n, int paired, int64_t *d_offsets,
                     int64_t *d_result, void *d_work, uint8_t *d_out, void *stream) {
    if (n_bytes < 0 || n < 0 || n > n_bytes) return ATR_ERR_INVALID;
    if (n_bytes >= (int64_t)0x7FFFFFF0ll) return ATR_ERR_UNSUPPORTED;          // (a record's text is at most twice its bytes)
    if (!d_offsets || !d_result) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long long used = paired ? (n & ~(int64_t)1) : n;
    if (used && (!d_bam || !d_starts || !d_work)) return ATR_ERR_INVALID;
    if (!d_out) {
        hipLaunchKernelGGL(bam_result_kernel, dim3(1), dim3(1), 0, st, (long long *)d_result, (long long *)d_offsets, used);
        if (used) {
            Workspace ws(d_work);
            const ScanWork<u64> w = scan_work<u64>(ws, used, 1);
            hipLaunchKernelGGL(bam_sizes_kernel, dim3(grid256(used)), dim3(256), 0, st, d_bam, d_starts, used, paired, w.sizes,
                               (long long *)d_result);
            device_scan(w.sizes, used, (u64 *)d_offsets, w.sums, (u64 *)d_offsets + used, st);
            hipLaunchKernelGGL(bam_total_kernel, dim3(1), dim3(1), 0, st, (const long long *)d_offsets, used, (long long *)d_result);
        }
        return launched("bam decode sizes launch");
    }
    if (used)
        hipLaunchKernelGGL(bam_emit_kernel, dim3((unsigned)blocks(used * BAM_EMIT_LANES, 256)), dim3(256), 0, st, d_bam,
                           d_starts, used, paired, (const long long *)d_offsets, d_out, (long long *)d_result);
    return launched("bam decode launch");
}

}  // extern "C"
