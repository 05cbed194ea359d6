// fastq_emit_kernels.hip -- the formatters of the device-resident FASTQ batch: atr_fastq_emit (records in input
// order), atr_fastq_emit_grouped (a stable partition by group) and atr_demux_groups (see include/atropos_hip.h,
// "device-resident FASTQ batch"; the per-record code is fastq_core.hpp and demux_core.hpp).
//
// Byte streaming like fastq_kernels.hip.  Every formatter runs twice: a sizing call (d_out null) gives every record
// its place with the exclusive scan of scan_kernels.hpp, the writing call puts the text there.  The staged formatter
// stages the contiguous byte span of a wave's records in LDS with coalesced 16-byte loads, lets every lane assemble
// its record in an LDS image of the output span, and writes that image with aligned 16-byte stores.
#include <hip/hip_runtime.h>

#include "atropos_hip.h"
#include "fastq_core.hpp"
#include "demux_core.hpp"

#include "fastq_device.hpp"
#include "launch_util.hpp"
#include "scan_kernels.hpp"

namespace atr {

// ------------------------------------------------------------------------- formatter
__global__ __launch_bounds__(256) void emit_sizes_kernel(const FastqRecord *__restrict__ records,
                                                         const int32_t *__restrict__ begin,
                                                         const int32_t *__restrict__ end,
                                                         const uint8_t *__restrict__ dest, int which, long long n,
                                                         uint32_t *__restrict__ sizes) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    uint32_t s = 0;
    if (!dest || dest[r] == which) s = fastq_record_bytes(records[r], max(0, end[r] - begin[r]));
    sizes[r] = s;
}

// One wave formats 64 consecutive records, one after the other, a byte per lane.
__global__ __launch_bounds__(256) void emit_kernel(const uint8_t *__restrict__ bytes,
                                                   const FastqRecord *__restrict__ records,
                                                   const int32_t *__restrict__ begin, const int32_t *__restrict__ end,
                                                   const int32_t *__restrict__ ubegin, const int32_t *__restrict__ uend,
                                                   const uint8_t *__restrict__ dest, int which, long long n,
                                                   const long long *__restrict__ offsets, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long r0 = tile * 64;
    if (r0 >= n) return;
    const int cnt = (int)min<long long>(64, n - r0);
    for (int i = 0; i < cnt; ++i) {
        const long long r = r0 + i;                               // wave-uniform
        if (dest && dest[r] != which) continue;
        const int a = begin[r], b = max(a, end[r]);
        fastq_format_record(out + offsets[r], bytes, records[r], a, b, ubegin ? ubegin[r] : a, uend ? uend[r] : b, lane, 64);
    }
}

// ---- staged formatter -------------------------------------------------------------------
// One wave formats a tile of EMIT_TILE consecutive records through LDS:
//   1. the tile's input span (first '@' .. end of the last quality line, ~10 KB for 150 bp
//      reads) is copied to LDS with coalesced 16-byte loads;
//   2. every lane pair assembles ITS record's output bytes at the record's place in an LDS image
//      of the tile's output span (LDS -> LDS, dword copies re-aligned in registers);
//   3. the image is written out with 16-byte stores aligned to the output buffer; the ragged
//      first / last bytes of the span with byte stores (neighbouring tiles never touch them).
// Output is never larger than input (same record layout, bases only removed), so one size
// bounds both stages.  Tiles that do not fit (very long names / reads) or whose records
// are not in file order take emit_kernel's path.
// Records per wave: 16; full-size stages (EMIT_STAGE, fastq_device.hpp) for records of more than ~400 bytes,
// half-size stages (twice the waves per CU: the kernel is latency bound) for short-read files; 32 records per
// wave with full stages when the caller gives no hint.
template <int EMIT_TILE, int STAGE = EMIT_STAGE>
__global__ __launch_bounds__(64) void emit_staged_kernel(const uint8_t *__restrict__ bytes,
                                                         const FastqRecord *__restrict__ records,
                                                         const int32_t *__restrict__ begin, const int32_t *__restrict__ end,
                                                         const int32_t *__restrict__ ubegin, const int32_t *__restrict__ uend,
                                                         const uint8_t *__restrict__ dest, int which, long long n,
                                                         const long long *__restrict__ offsets, uint8_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_emit[];
    uint8_t *s_in = s_emit, *s_out = s_emit + STAGE;
    constexpr int LPR = 64 / EMIT_TILE;                       // lanes per record (the first two do the work)
    const int lane = threadIdx.x, slot = lane / LPR, part = lane % LPR;
    const long long r0 = (long long)blockIdx.x * EMIT_TILE;
    const int cnt = (int)min<long long>(EMIT_TILE, n - r0);
    const long long r = r0 + slot;
    const bool live = slot < cnt;
    FastqRecord rec = {0, 0, 0, 0, 0, 0, 0, 0};
    int a = 0, b = 0, ub = 0, ue = 0;
    long long off = 0;
    bool keep = false;
    if (live) {
        rec = records[r];
        a = begin[r];
        b = max(a, end[r]);
        ub = ubegin ? ubegin[r] : a;
        ue = uend ? uend[r] : b;
        off = offsets[r];
        keep = !dest || dest[r] == which;
    }
    const uint32_t rec_lo = rec.name_off - 1u, rec_hi = rec.qual_off + rec.qual_len;     // '@' .. last quality byte
    const uint32_t in_lo = __shfl(rec_lo, 0, 64), in_hi = __shfl(rec_hi, LPR * (cnt - 1), 64);
    const long long out_lo = offsets[r0], out_hi = offsets[r0 + cnt];
    const bool ordered = __all(!live || (rec_lo >= in_lo && rec_hi <= in_hi && rec.seq_off >= rec_lo &&
                                         rec.seq_off + rec.seq_len <= rec.qual_off && rec.name_off + rec.name_len <= rec.seq_off &&
                                         !(rec.flags & 2u)));
    const uint32_t mis_in = in_lo & 15u, mis_out = (uint32_t)(out_lo & 15);
    const bool fits = ordered && (in_hi - in_lo) + mis_in + 16u <= (uint32_t)STAGE &&
                      (uint32_t)(out_hi - out_lo) + mis_out + 16u <= (uint32_t)STAGE;
    if (out_hi == out_lo) return;
    if (!fits) {                                           // slow path: a byte per lane straight from / to global
        for (int i = 0; i < cnt; ++i) {
            const long long ri = r0 + i;
            if (dest && dest[ri] != which) continue;
            const int ai = begin[ri], bi = max(ai, end[ri]);
            fastq_format_record(out + offsets[ri], bytes, records[ri], ai, bi, ubegin ? ubegin[ri] : ai, uend ? uend[ri] : bi,
                                lane, 64);
        }
        return;
    }
    // 1. stage the input span
    {
        const uint8_t *src_al = bytes + (in_lo - mis_in);
        const uint32_t need = in_hi - in_lo + mis_in;
        for (uint32_t o = (uint32_t)lane * 16u; o < need; o += 64u * 16u) *(uint4 *)(s_in + o) = *(const uint4 *)(src_al + o);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // 2. two lanes format one record inside the output image: the even lane "@name\nSEQ\n",
    //    the odd lane "+[name]\nQUAL\n"
    if (keep) {
        const uint8_t *in = s_in + mis_in;                  // in[x - in_lo] = bytes[x]
        uint8_t *o = s_out + mis_out + (uint32_t)(off - out_lo);
        const uint32_t kept = (uint32_t)(b - a);
        if (part == 0) {
            *o++ = '@';
            lds_copy(o, in + (rec.name_off - in_lo), rec.name_len);
            o += rec.name_len;
            *o++ = '\n';
            const uint8_t *sq = in + (rec.seq_off - in_lo) + a;
            if (ub <= a && ue >= b) {
                lds_copy(o, sq, kept);
            } else {
                for (uint32_t k = 0; k < kept; ++k) {
                    const int pos = a + (int)k;
                    o[k] = (pos >= ub && pos < ue) ? sq[k] : (uint8_t)'N';
                }
            }
            o[kept] = '\n';
        } else if (part == 1) {
            o += 1u + rec.name_len + 1u + kept + 1u;
            *o++ = '+';
            if (rec.flags & 1u) { lds_copy(o, in + (rec.name_off - in_lo), rec.name_len); o += rec.name_len; }
            *o++ = '\n';
            lds_copy(o, in + (rec.qual_off - in_lo) + a, kept);
            o[kept] = '\n';
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // 3. write the image: aligned 16-byte blocks, byte stores at the ragged ends
    {
        uint8_t *dst_al = out + (out_lo - mis_out);          // 16-byte aligned when `out` is
        const uint32_t lo = mis_out, hi = mis_out + (uint32_t)(out_hi - out_lo);
        for (uint32_t o = (uint32_t)lane * 16u; o < hi; o += 64u * 16u) {
            if (o >= lo && o + 16u <= hi) {
                *(uint4 *)(dst_al + o) = *(const uint4 *)(s_out + o);
            } else {
                for (uint32_t k = max(o, lo); k < min(o + 16u, hi); ++k) dst_al[k] = s_out[k];
            }
        }
    }
}

// ---- grouped formatter ------------------------------------------------------------------
// atr_fastq_emit_grouped: the records of group 0 first, then group 1's ..., input order inside a group -- a
// stable partition by group with a byte-weighted prefix, in one pass over the records per call:
//   sizing:  group_hist_kernel     bytes per (group, block of 256 records), summed in LDS
//            device_scan           exclusive 64-bit scan of that matrix, group-major: entry (g, b) becomes the
//                                  position of the first byte block b adds to group g
//            group_offsets_kernel  the position of every record: matrix entry + the bytes the earlier records
//                                  of its block add to its group
//   writing: emit_grouped_kernel   every wave formats its 64 records, each at its position
// No global atomics: the positions do not depend on the launch shape or on timing.
constexpr int GRP_BLOCK = 256;

__device__ __forceinline__ uint32_t grouped_load(const FastqRecord *records, const int32_t *begin, const int32_t *end,
                                                 const int32_t *group, int n_groups, long long r, long long n, int &g) {
    g = -1;
    if (r >= n) return 0u;
    g = group[r];
    return demux_record_bytes(records[r], begin[r], end[r], g, n_groups);
}

// LDS: n_groups uint32
__global__ __launch_bounds__(GRP_BLOCK) void group_hist_kernel(const FastqRecord *__restrict__ records,
                                                               const int32_t *__restrict__ begin,
                                                               const int32_t *__restrict__ end,
                                                               const int32_t *__restrict__ group, int n_groups, long long n,
                                                               long long nb, uint32_t *__restrict__ hist) {
    extern __shared__ uint32_t s_hist[];
    for (int i = threadIdx.x; i < n_groups; i += GRP_BLOCK) s_hist[i] = 0u;
    __syncthreads();
    int g;
    const uint32_t s = grouped_load(records, begin, end, group, n_groups, (long long)blockIdx.x * GRP_BLOCK + threadIdx.x, n, g);
    if (g >= 0) atomicAdd(&s_hist[g], s);                       // (integer sums in LDS: the order does not show)
    __syncthreads();
    for (int i = threadIdx.x; i < n_groups; i += GRP_BLOCK) hist[(long long)i * nb + blockIdx.x] = s_hist[i];
}

// LDS: (GRP_BLOCK / 64) x n_groups uint32 -- what every wave of the block adds to every group
__global__ __launch_bounds__(GRP_BLOCK) void group_offsets_kernel(const FastqRecord *__restrict__ records,
                                                                  const int32_t *__restrict__ begin,
                                                                  const int32_t *__restrict__ end,
                                                                  const int32_t *__restrict__ group, int n_groups, long long n,
                                                                  long long nb, const long long *__restrict__ base,
                                                                  long long *__restrict__ offsets,
                                                                  long long *__restrict__ group_offsets) {
    extern __shared__ uint32_t s_wave[];
    for (int i = threadIdx.x; i < (GRP_BLOCK / 64) * n_groups; i += GRP_BLOCK) s_wave[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * GRP_BLOCK + threadIdx.x;
    int g;
    const uint32_t s = grouped_load(records, begin, end, group, n_groups, r, n, g);
    // the distinct groups of the wave, one after the other: the lanes of the leader's group take the prefix of
    // their sizes in lane order (= input order), the leader notes the group's total
    uint32_t before = 0u;
    unsigned long long todo = __ballot(g >= 0);
    while (todo) {                                              // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int lg = __shfl(g, leader, 64);
        const bool mine = g == lg;
        uint32_t x = mine ? s : 0u;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (mine) before = x - s;
        const uint32_t total = __shfl(x, 63, 64);
        if (lane == leader) s_wave[wave * n_groups + lg] = total;
        todo &= ~__ballot(mine);
    }
    __syncthreads();
    if (r < n) {
        long long pos = -1;                                     // a record that is not written has no position
        if (g >= 0) {
            pos = base[(long long)g * nb + blockIdx.x] + (long long)before;
            for (int w = 0; w < wave; ++w) pos += (long long)s_wave[w * n_groups + g];
        }
        offsets[r] = pos;
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < n_groups; i += GRP_BLOCK) group_offsets[i] = base[(long long)i * nb];
}

// One wave formats 64 consecutive records: every lane fetches the state of one, then the wave writes them one
// after the other with fastq_format_record, a byte per lane (neighbours go to different places of the buffer,
// so there is no output span to stage as emit_staged_kernel does).
__global__ __launch_bounds__(256) void emit_grouped_kernel(const uint8_t *__restrict__ bytes,
                                                           const FastqRecord *__restrict__ records,
                                                           const int32_t *__restrict__ begin, const int32_t *__restrict__ end,
                                                           const int32_t *__restrict__ ubegin, const int32_t *__restrict__ uend,
                                                           const int32_t *__restrict__ group, int n_groups, long long n,
                                                           const long long *__restrict__ offsets, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;
    FastqRecord rec = {0, 0, 0, 0, 0, 0, 0, 0};
    int a = 0, b = 0, ub = 0, ue = 0;
    long long off = -1;
    if (r < n) {
        const int g = group[r];
        if (g >= 0 && g < n_groups) {
            rec = records[r];
            a = begin[r];
            b = max(a, end[r]);
            ub = ubegin ? ubegin[r] : a;
            ue = uend ? uend[r] : b;
            off = offsets[r];
        }
    }
    unsigned long long todo = __ballot(off >= 0);
    while (todo) {                                              // wave-uniform
        const int i = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        FastqRecord rc;
        rc.name_off = __shfl(rec.name_off, i, 64); rc.name_len = __shfl(rec.name_len, i, 64);
        rc.seq_off = __shfl(rec.seq_off, i, 64); rc.seq_len = __shfl(rec.seq_len, i, 64);
        rc.qual_off = __shfl(rec.qual_off, i, 64); rc.qual_len = __shfl(rec.qual_len, i, 64);
        rc.flags = __shfl(rec.flags, i, 64); rc.reserved = __shfl(rec.reserved, i, 64);
        const long long oi = __shfl(off, i, 64);
        fastq_format_record(out + oi, bytes, rc, __shfl(a, i, 64), __shfl(b, i, 64), __shfl(ub, i, 64), __shfl(ue, i, 64),
                            lane, 64);
    }
}

__global__ __launch_bounds__(256) void demux_groups_kernel(const uint8_t *__restrict__ dest, const uint8_t *__restrict__ matched,
                                                           const long long *__restrict__ which,
                                                           const int32_t *__restrict__ adapter_group, int n_adapters,
                                                           int untrimmed_group, long long n, int32_t *__restrict__ group) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    group[r] = demux_group_one(dest[r], matched[r] != 0, which[r], adapter_group, n_adapters, untrimmed_group);
}

namespace {

// work layout of the grouped sizing: [hist u32 x cells][base u64 x cells][sums u64 x scan_blocks(cells)],
// cells = n_groups * nb, nb = blocks of GRP_BLOCK records.  `base` has no slot for the total.
struct GroupedWork {
    long long nb, cells;
    uint32_t *hist;
    u64 *base, *sums;
    size_t bytes;
};

inline GroupedWork grouped_work(void *work, long long n, int n_groups) {
    GroupedWork w;
    Workspace ws(work);
    w.nb = blocks(n, GRP_BLOCK);
    w.cells = (long long)n_groups * w.nb;
    w.hist = ws.take<uint32_t>((size_t)w.cells);
    w.base = ws.take<u64>((size_t)w.cells);
    w.sums = ws.take<u64>((size_t)scan_blocks(w.cells));
    w.bytes = ws.bytes();
    return w;
}

}  // namespace
}  // namespace atr

using namespace atr;

extern "C" {

// work layout: scan_work of uint32 sizes
size_t atr_fastq_emit_work_bytes(int64_t n) { return n < 0 ? 0 : scan_work_bytes<uint32_t>(n); }

int atr_fastq_emit(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                   const int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end,
                   const uint8_t *d_dest, int dest, int64_t n, int record_bytes_hint, int64_t *d_offsets, void *d_work,
                   uint8_t *d_out, void *stream) {
    if (n < 0 || !d_offsets || ((d_unmasked_begin == nullptr) != (d_unmasked_end == nullptr))) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (!d_out) hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_offsets, 0ll);
        return launched("fastq emit launch");
    }
    if (!d_bytes || !d_records || !d_begin || !d_end || !d_work) return ATR_ERR_INVALID;
    if (!d_out) {
        Workspace ws(d_work);
        const ScanWork<uint32_t> w = scan_work<uint32_t>(ws, n);
        hipLaunchKernelGGL(emit_sizes_kernel, dim3(grid256(n)), dim3(256), 0, st, (const FastqRecord *)d_records, d_begin,
                           d_end, d_dest, dest, (long long)n, w.sizes);
        device_scan(w.sizes, n, (u64 *)d_offsets, w.sums, (u64 *)d_offsets + n, st);
        return launched("fastq emit sizes launch");
    }
    const long long ntiles = (n + 63) / 64;
    if (((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_bytes & 15) == 0) {
        if (record_bytes_hint > 400)
            hipLaunchKernelGGL(emit_staged_kernel<16>, dim3((unsigned)((n + 15) / 16)), dim3(64), 2 * EMIT_STAGE, st, d_bytes,
                               (const FastqRecord *)d_records, d_begin, d_end, d_unmasked_begin, d_unmasked_end, d_dest,
                               dest, (long long)n, (const long long *)d_offsets, d_out);
        else if (record_bytes_hint > 0 && record_bytes_hint <= 380)   // 8 records, 2 x 3.25 KB per wave: 24 waves per CU (-5 % more)
            hipLaunchKernelGGL((emit_staged_kernel<8, EMIT_STAGE / 4>), dim3((unsigned)((n + 7) / 8)), dim3(64), EMIT_STAGE / 2, st, d_bytes,
                               (const FastqRecord *)d_records, d_begin, d_end, d_unmasked_begin, d_unmasked_end, d_dest,
                               dest, (long long)n, (const long long *)d_offsets, d_out);
        else if (record_bytes_hint > 0)                    // short records: half-size tiles and stages, 12 waves per CU (-15 %)
            hipLaunchKernelGGL((emit_staged_kernel<16, EMIT_STAGE / 2>), dim3((unsigned)((n + 15) / 16)), dim3(64), EMIT_STAGE, st, d_bytes,
                               (const FastqRecord *)d_records, d_begin, d_end, d_unmasked_begin, d_unmasked_end, d_dest,
                               dest, (long long)n, (const long long *)d_offsets, d_out);
        else
            hipLaunchKernelGGL(emit_staged_kernel<32>, dim3((unsigned)((n + 31) / 32)), dim3(64), 2 * EMIT_STAGE, st, d_bytes,
                               (const FastqRecord *)d_records, d_begin, d_end, d_unmasked_begin, d_unmasked_end, d_dest,
                               dest, (long long)n, (const long long *)d_offsets, d_out);
        return launched("emit_staged_kernel launch");
    }
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, st, d_bytes,
                       (const FastqRecord *)d_records, d_begin, d_end, d_unmasked_begin, d_unmasked_end, d_dest, dest,
                       (long long)n, (const long long *)d_offsets, d_out);
    return launched("emit_kernel launch");
}

size_t atr_fastq_emit_grouped_work_bytes(int64_t n, int n_groups) {
    if (n < 0 || n_groups < 1 || n_groups > ATR_EMIT_MAX_GROUPS) return 0;
    return grouped_work(nullptr, n, n_groups).bytes;
}

int atr_fastq_emit_grouped(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                           const int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end,
                           const int32_t *d_group, int n_groups, int64_t n, int record_bytes_hint, int64_t *d_offsets,
                           int64_t *d_group_offsets, void *d_work, uint8_t *d_out, void *stream) {
    (void)record_bytes_hint;
    if (n_groups > ATR_EMIT_MAX_GROUPS) return ATR_ERR_UNSUPPORTED;
    if (n < 0 || n_groups < 1 || !d_group_offsets || ((d_unmasked_begin == nullptr) != (d_unmasked_end == nullptr)))
        return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (!d_out) {
            hipError_t me = hipMemsetAsync(d_group_offsets, 0, (size_t)(n_groups + 1) * 8, st);
            if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync");
        }
        return ATR_OK;
    }
    if (!d_bytes || !d_records || !d_begin || !d_end || !d_group || !d_offsets || !d_work) return ATR_ERR_INVALID;
    const FastqRecord *records = (const FastqRecord *)d_records;
    if (!d_out) {
        const GroupedWork w = grouped_work(d_work, n, n_groups);
        hipLaunchKernelGGL(group_hist_kernel, dim3((unsigned)w.nb), dim3(GRP_BLOCK), (size_t)n_groups * 4, st, records, d_begin,
                           d_end, d_group, n_groups, (long long)n, w.nb, w.hist);
        device_scan(w.hist, w.cells, w.base, w.sums, (u64 *)d_group_offsets + n_groups, st);
        hipLaunchKernelGGL(group_offsets_kernel, dim3((unsigned)w.nb), dim3(GRP_BLOCK), (size_t)(GRP_BLOCK / 64) * n_groups * 4,
                           st, records, d_begin, d_end, d_group, n_groups, (long long)n, w.nb, (const long long *)w.base,
                           (long long *)d_offsets, (long long *)d_group_offsets);
        return launched("fastq grouped emit sizes launch");
    }
    hipLaunchKernelGGL(emit_grouped_kernel, dim3(grid256(n)), dim3(256), 0, st, d_bytes, records, d_begin, d_end,
                       d_unmasked_begin, d_unmasked_end, d_group, n_groups, (long long)n, (const long long *)d_offsets, d_out);
    return launched("emit_grouped_kernel launch");
}

int atr_demux_groups(const uint8_t *d_dest, const uint8_t *d_matched, const int64_t *d_last_which,
                     const int32_t *d_adapter_group, int n_adapters, int untrimmed_group, int64_t n, int32_t *d_group,
                     void *stream) {
    if (n < 0 || n_adapters < 0) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_dest || !d_matched || !d_last_which || !d_group) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(demux_groups_kernel, dim3(grid256(n)), dim3(256), 0, (hipStream_t)stream, d_dest, d_matched,
                       (const long long *)d_last_which, d_adapter_group, n_adapters, untrimmed_group, (long long)n, d_group);
    return launched("demux_groups_kernel launch");
}

}  // extern "C"
