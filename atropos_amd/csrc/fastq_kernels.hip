// fastq_kernels.hip -- the device-resident FASTQ batch: line index, record descriptors,
// 4-bit pack straight from the file bytes, interval-update trimmers, filters and the
// formatter (see include/atropos_hip.h, "device-resident FASTQ batch").
//
// All of this is byte streaming: every kernel is bound by HBM traffic or by the number of
// scattered byte accesses, none has arithmetic worth speaking of.  Layout decisions:
//   * the file chunk stays as it came off the disk; records are 32-byte descriptors
//     (offsets into the chunk), modifier state is two int32 per read;
//   * line ends are found with 16-byte loads + a SWAR zero-byte test, positions come from
//     a two-level exclusive scan (no atomics, input order preserved);
//   * the packer copies each sequence line into an LDS row with one direct-to-LDS load
//     (global_load_lds_dword) and lets every lane re-align its row in registers (v_alignbyte_b32);
//   * the formatter stages the contiguous byte span of a wave's 64 records in LDS with
//     coalesced 16-byte loads, lets every lane assemble its record in an LDS image of the
//     output span, and writes that image with aligned 16-byte stores.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>

#include "atropos_hip.h"
#include "locate_core.hpp"
#include "fastq_core.hpp"
#include "misc_core.hpp"
#include "demux_core.hpp"
#include "pairtext_core.hpp"

#include "pack_fast.hpp"

namespace atr {

int hip_fail(hipError_t e, const char *what);             // api.hip

// ------------------------------------------------------------------------- scans
constexpr int SCAN_BLOCK = 1024;

// inclusive scan of one value per thread over a 1024-thread block; returns the inclusive
// prefix, *total = block sum
__device__ __forceinline__ unsigned long long block_scan_1024(unsigned long long v, unsigned long long *s_part,
                                                               unsigned long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) s_part[wave] = x;
    __syncthreads();
    if (wave == 0) {
        unsigned long long w = lane < (SCAN_BLOCK / 64) ? s_part[lane] : 0ull;
#pragma unroll
        for (int off = 1; off < SCAN_BLOCK / 64; off <<= 1) {
            const unsigned long long y = __shfl_up(w, off, 64);
            if (lane >= off) w += y;
        }
        if (lane < SCAN_BLOCK / 64) s_part[lane] = w;
    }
    __syncthreads();
    const unsigned long long base = wave ? s_part[wave - 1] : 0ull;
    *total = s_part[SCAN_BLOCK / 64 - 1];
    return x + base;
}

// level 1: out[i] = exclusive prefix of v inside its block of 1024, sums[b] = block total
__global__ __launch_bounds__(SCAN_BLOCK) void scan_local_kernel(const uint32_t *__restrict__ v, long long n,
                                                                 long long *__restrict__ out,
                                                                 unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long s_part[SCAN_BLOCK / 64];
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const unsigned long long x = i < n ? v[i] : 0u;
    unsigned long long total;
    const unsigned long long inc = block_scan_1024(x, s_part, &total);
    if (i < n) out[i] = (long long)(inc - x);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// level 2: exclusive scan of the nb block totals in place (one block; a thread owns a run)
__global__ __launch_bounds__(SCAN_BLOCK) void scan_sums_kernel(unsigned long long *__restrict__ sums, long long nb,
                                                                long long *__restrict__ total_out) {
    __shared__ unsigned long long s_part[SCAN_BLOCK / 64];
    const long long per = (nb + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const long long lo = min(nb, per * (long long)threadIdx.x), hi = min(nb, lo + per);
    unsigned long long mine = 0;
    for (long long i = lo; i < hi; ++i) mine += sums[i];
    unsigned long long total;
    const unsigned long long inc = block_scan_1024(mine, s_part, &total);
    unsigned long long run = inc - mine;
    for (long long i = lo; i < hi; ++i) { const unsigned long long t = sums[i]; sums[i] = run; run += t; }
    if (threadIdx.x == 0 && total_out) *total_out = (long long)total;
}

// level 3: add the block bases; out[n] = grand total
__global__ __launch_bounds__(SCAN_BLOCK) void scan_add_kernel(long long *__restrict__ out, long long n,
                                                               const unsigned long long *__restrict__ sums,
                                                               long long nb) {
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    if (i < n) out[i] += (long long)sums[blockIdx.x];
}

// ------------------------------------------------------------------------- line index
constexpr int NL_THREADS = 256, NL_BLOCK_BYTES = NL_THREADS * 16;

// one bit per byte of a dword: 0x80 in every byte equal to c, gathered into the low 4 bits
__device__ __forceinline__ uint32_t byte_eq_mask4(uint32_t w, uint32_t crep) {
    const uint32_t x = w ^ crep;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);     // 0x80 in every zero byte
    const uint32_t m = z >> 7;
    return (m | (m >> 7) | (m >> 14) | (m >> 21)) & 0xFu;
}

// bit i set <=> byte i of the 16 bytes at `off` ends a line (universal newlines: "\n", or a
// "\r" that is not followed by "\n"); bytes at or beyond nbytes are masked out
__device__ __forceinline__ uint32_t newline_mask16(const uint8_t *bytes, long long off, long long nbytes, bool &saw_cr) {
    saw_cr = false;
    if (off >= nbytes) return 0u;
    const uint4 v = *(const uint4 *)(bytes + off);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t nl = 0, anycr = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        nl |= byte_eq_mask4(w[d], 0x0A0A0A0Au) << (4 * d);
        const uint32_t x = w[d] ^ 0x0D0D0D0Du;
        anycr |= (x - 0x01010101u) & ~x & 0x80808080u;          // nonzero <=> some byte of the dword is '\r'
    }
    uint32_t cr = 0;
    if (anycr) {                                                // rare (no '\r' at all in Unix files)
        saw_cr = true;
#pragma unroll
        for (int d = 0; d < 4; ++d) cr |= byte_eq_mask4(w[d], 0x0D0D0D0Du) << (4 * d);
        // a '\r' ends a line unless a '\n' follows
        const uint32_t next_nl = (off + 16 < nbytes && bytes[off + 16] == '\n') ? 1u : 0u;
        cr &= ~((nl >> 1) | (next_nl << 15));
    }
    uint32_t mask = nl | cr;
    const long long valid = nbytes - off;
    if (valid < 16) mask &= (1u << valid) - 1u;
    return mask;
}

__global__ __launch_bounds__(NL_THREADS) void count_newlines_kernel(const uint8_t *__restrict__ bytes, long long nbytes,
                                                                     uint32_t *__restrict__ block_counts,
                                                                     uint32_t *__restrict__ has_cr) {
    __shared__ uint32_t s_cnt[NL_THREADS / 64];
    const long long off = ((long long)blockIdx.x * NL_THREADS + threadIdx.x) * 16;
    bool saw_cr;
    uint32_t c = __popc(newline_mask16(bytes, off, nbytes, saw_cr));
    if (__any(saw_cr) && (threadIdx.x & 63) == 0) atomicOr(has_cr, 1u);    // the chunk holds '\r': records check for "\r\n"
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(NL_THREADS) void line_ends_kernel(const uint8_t *__restrict__ bytes, long long nbytes,
                                                                const long long *__restrict__ block_base,
                                                                uint32_t *__restrict__ line_ends) {
    __shared__ uint32_t s_cnt[NL_THREADS / 64];
    const long long off = ((long long)blockIdx.x * NL_THREADS + threadIdx.x) * 16;
    bool saw_cr;
    uint32_t mask = newline_mask16(bytes, off, nbytes, saw_cr);
    const uint32_t c = __popc(mask);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_cnt[wave] = x;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += s_cnt[w];
    long long slot = block_base[blockIdx.x] + base + (x - c);
    while (mask) {
        const int b = __ffs((int)mask) - 1;
        mask &= mask - 1;
        line_ends[slot++] = (uint32_t)(off + b);
    }
}

__global__ __launch_bounds__(256) void records_kernel(const uint8_t *__restrict__ bytes,
                                                      const uint32_t *__restrict__ line_ends, long long nrec,
                                                      const uint32_t *__restrict__ has_cr,
                                                      FastqRecord *__restrict__ records,
                                                      unsigned long long *__restrict__ error) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec) return;
    FastqRecord rec;
    const int err = fastq_record_one(bytes, line_ends, r, *has_cr != 0, rec);
    records[r] = rec;
    if (err) atomicMin(error, (unsigned long long)r * 8ull + (unsigned long long)err);
}

__global__ void set_i64_kernel(long long *p, long long v) { *p = v; }

// ------------------------------------------------------------------------- pack from records
struct PackTable256 { uint8_t t[256]; };


// The sequence lines sit at arbitrary byte offsets of the file chunk, ~300 bytes apart.  A
// wave first copies the aligned dwords of its 64 lines into 64 LDS rows -- one
// global_load_lds_dword per line, lanes = consecutive dwords, so every line is fetched as one
// contiguous burst and the 64 copies are all in flight together (no VGPR round trip) -- and
// then every lane packs its own row, re-aligning the dwords with v_alignbyte_b32.
// Row stride is odd (in dwords): lanes reading dword d of their own rows hit 64 different banks.
__device__ __forceinline__ void glds_dword(const uint8_t *gsrc, uint32_t *lds_dst_wave_uniform) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)lds_dst_wave_uniform, 4, 0, 0);
}

template <bool PLANES>
__global__ void pack_records_kernel(
    const uint8_t *__restrict__ bytes, const FastqRecord *__restrict__ records, const int32_t *__restrict__ begin,
    const int32_t *__restrict__ end, long long nreads, int max_len, int nchunks, int stride_dw, const PackTable256 tab,
    uint4 *__restrict__ packed, int32_t *__restrict__ lens, int32_t *__restrict__ invalid) {
    __shared__ uint8_t s_tab[256];
    __shared__ uint32_t s_spread[PLANES ? 256 : 1];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_rows[];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        s_tab[i] = tab.t[i];
        if (PLANES) s_spread[i] = spread_code((uint32_t)tab.t[i] & 15u);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const long long tile = (long long)blockIdx.x * waves + wave;
    const long long ntiles = (nreads + 63) >> 6;
    if (tile >= ntiles) return;
    const long long r = tile * 64 + lane;
    uint32_t soff = 0;
    int n = 0;
    if (r < nreads) {
        const FastqRecord rec = records[r];
        int a = begin ? begin[r] : 0, b = end ? end[r] : (int)rec.seq_len;
        a = max(0, min(a, (int)rec.seq_len));
        b = max(a, min(b, (int)rec.seq_len));
        soff = rec.seq_off + (uint32_t)a;
        n = min(b - a, max_len);
        if (lens) lens[r] = n;
    }
    const uint32_t sh = soff & 3u;
    const int nd = (n + (int)sh + 3) >> 2;                      // aligned dwords that hold the read
    uint32_t *rows = s_rows + (size_t)wave * 64 * stride_dw;
    const int cnt = (int)min<long long>(64, nreads - tile * 64);
    for (int i = 0; i < cnt; ++i) {                             // wave-uniform: row i <- line i
        const uint32_t so = (uint32_t)__builtin_amdgcn_readlane((int)(soff - sh), i);
        const int nd_i = __builtin_amdgcn_readlane(nd, i);
        for (int d0 = 0; d0 < nd_i; d0 += 64)
            if (d0 + lane < nd_i) glds_dword(bytes + so + (size_t)(d0 + lane) * 4, rows + (size_t)i * stride_dw + d0);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const uint32_t *p = rows + (size_t)lane * stride_dw;
    uint4 *dst = packed + (size_t)tile * nchunks * 64 + lane;
    bool zero_seen = false;
    // four bases per step out of the lane's LDS row (pack_fast.hpp); dwords from nd on are not read
    if (PLANES) pack_planes_row_fast(p, 0u, (uint32_t)nd, sh, n, nchunks, s_tab, dst, zero_seen);
    else pack_codes_row_fast(p, 0u, (uint32_t)nd, sh, n, nchunks, s_tab, dst, zero_seen);
    if (invalid && zero_seen) atomicAdd(invalid, 1);
}

// ------------------------------------------------------------------------- interval updates
__device__ __forceinline__ bool load_interval(const FastqRecord *records, const int32_t *begin, const int32_t *end,
                                              long long r, FastqRecord &rec, int &a, int &b) {
    rec = records[r];
    a = begin[r];
    b = end[r];
    return b > a;
}

__global__ __launch_bounds__(256) void clip_kernel(const FastqRecord *__restrict__ records, int32_t *__restrict__ begin,
                                                   int32_t *__restrict__ end, long long n, int front, int back) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int a = begin[r], b = end[r];
    if (b <= a || (front == 0 && back == 0)) return;          // Trimmer.clip: (front or back) and len(read) > 0
    int na, nb;
    py_clip(b - a, front, back, back < 0, na, nb);            // read[front:back] or read[front:]
    begin[r] = a + na;
    end[r] = a + nb;
}

__global__ __launch_bounds__(256) void quality_trim_kernel(const uint8_t *__restrict__ bytes,
                                                           const FastqRecord *__restrict__ records,
                                                           int32_t *__restrict__ begin, int32_t *__restrict__ end,
                                                           long long n, int cutoff_front, int cutoff_back, int base,
                                                           int nextseq) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    FastqRecord rec;
    int a, b;
    if (!load_interval(records, begin, end, r, rec, a, b)) return;       // if len(read) == 0: return read
    const uint8_t *qual = bytes + rec.qual_off + a;
    if (nextseq) {
        const int stop = nextseq_trim_one(bytes + rec.seq_off + a, qual, b - a, cutoff_back, base);
        end[r] = a + stop;                                                // subseq(read, end=stop)
    } else {
        int s, e;
        quality_trim_one(bytes, rec.qual_off + (uint32_t)a, b - a, cutoff_front, cutoff_back, base, s, e);
        begin[r] = a + s;
        end[r] = a + e;
    }
}

__global__ __launch_bounds__(256) void nend_trim_kernel(const uint8_t *__restrict__ bytes,
                                                        const FastqRecord *__restrict__ records,
                                                        int32_t *__restrict__ begin, int32_t *__restrict__ end,
                                                        const int32_t *__restrict__ ubegin,
                                                        const int32_t *__restrict__ uend, long long n) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    FastqRecord rec;
    int a, b;
    if (!load_interval(records, begin, end, r, rec, a, b)) return;
    const int ub = ubegin ? ubegin[r] - a : 0, ue = uend ? uend[r] - a : b - a;
    int s, e;
    nend_trim_one(bytes + rec.seq_off + a, b - a, ub, ue, s, e);
    begin[r] = a + s;
    end[r] = a + (e < s ? s : e);
}

__global__ __launch_bounds__(256) void match_trim_kernel(const int16_t *__restrict__ matches,
                                                         const uint8_t *__restrict__ front, int default_front,
                                                         int32_t *__restrict__ begin, int32_t *__restrict__ end,
                                                         uint8_t *__restrict__ active, uint8_t *__restrict__ matched,
                                                         long long n) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    if (active && !active[r]) return;
    const int16_t *m = matches + 8 * r;
    if (m[1] < 0) { if (active) active[r] = 0; return; }
    const int rstart = m[2], rstop = m[3];
    int f = front ? (int)front[r] : default_front;
    if (f > 1) f = rstart == 0 ? 1 : 0;                                   // Match: front guessed from rstart == 0
    const int a = begin[r], b = end[r];
    if (f) begin[r] = min(b, a + rstop);                                  // read[match.rstop:]
    else end[r] = max(a, min(b, a + rstart));                             // read[:match.rstart]
    if (matched) matched[r] = 1;
}

__global__ __launch_bounds__(256) void read_filter_kernel(const uint8_t *__restrict__ bytes,
                                                          const FastqRecord *__restrict__ records,
                                                          const int32_t *__restrict__ begin,
                                                          const int32_t *__restrict__ end,
                                                          const int32_t *__restrict__ ubegin,
                                                          const int32_t *__restrict__ uend,
                                                          const uint8_t *__restrict__ matched, long long n, int min_len,
                                                          int max_len, double max_n, int discard_trimmed,
                                                          int discard_untrimmed, uint8_t *__restrict__ dest,
                                                          uint8_t *__restrict__ fail_mask) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const FastqRecord rec = records[r];
    const int a = begin[r], b = max(a, end[r]);
    const int ub = ubegin ? ubegin[r] - a : 0, ue = uend ? uend[r] - a : b - a;
    const uint32_t mask = read_filter_mask(bytes + rec.seq_off + a, b - a, ub, ue, matched ? matched[r] != 0 : false,
                                           min_len, max_len, max_n, discard_trimmed, discard_untrimmed);
    if (dest) dest[r] = (uint8_t)filter_destination(mask, 0u, false, 1);
    if (fail_mask) fail_mask[r] = (uint8_t)mask;
}

__global__ __launch_bounds__(256) void pair_filter_kernel(const uint8_t *__restrict__ mask1,
                                                          const uint8_t *__restrict__ mask2, long long n,
                                                          int min_affected, uint8_t *__restrict__ dest) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    dest[r] = (uint8_t)filter_destination(mask1[r], mask2[r], true, min_affected);
}

struct CompTable256 { uint8_t c[256]; };

__global__ __launch_bounds__(256) void insert_plan_kernel(
    const int16_t *__restrict__ ins, const int16_t *__restrict__ fb1, const int16_t *__restrict__ fb2,
    uint8_t *bytes1, const FastqRecord *__restrict__ records1, uint8_t *bytes2, const FastqRecord *__restrict__ records2,
    int32_t *__restrict__ begin1, int32_t *__restrict__ end1, int32_t *__restrict__ begin2, int32_t *__restrict__ end2,
    int32_t *__restrict__ uend1, int32_t *__restrict__ uend2, long long n, int min_insert_len, int symmetric,
    int trim_action, int correct_action, int min_qual_diff, const CompTable256 ct, uint8_t *__restrict__ matched1,
    uint8_t *__restrict__ matched2, int32_t *__restrict__ corrected, unsigned long long *__restrict__ error) {
    __shared__ uint8_t s_comp[256];
    s_comp[threadIdx.x] = ct.c[threadIdx.x];
    __syncthreads();
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int a1 = begin1[r], a2 = begin2[r];
    int len1 = max(0, end1[r] - a1), len2 = max(0, end2[r] - a2);
    InsertPlan P;
    insert_plan_matches(ins + 24 * r, fb1 + 8 * r, fb2 + 8 * r, len1, len2, min_insert_len, symmetric, correct_action >= 0, P);
    if (corrected) corrected[2 * r] = corrected[2 * r + 1] = 0;
    if (P.correct) {                                                   // correct_errors(..., truncate_seqs=True), :448-449
        const FastqRecord r1 = records1[r], r2 = records2[r];
        int32_t changed[2], newlen[2];
        correct_errors_one(bytes1 + r1.seq_off + a1, bytes1 + r1.qual_off + a1, len1, bytes2 + r2.seq_off + a2,
                           bytes2 + r2.qual_off + a2, len2, P.corr, correct_action, min_qual_diff, true, s_comp, changed,
                           newlen);
        if (changed[0] < 0) {
            atomicMin(error, (unsigned long long)r * 8ull + (unsigned long long)(-changed[0]));
        } else {
            len1 = newlen[0]; len2 = newlen[1];
            end1[r] = a1 + len1; end2[r] = a2 + len2;
            if (corrected) { corrected[2 * r] = changed[0]; corrected[2 * r + 1] = changed[1]; }
        }
    }
    int cut1, cut2;
    bool m1, m2;
    insert_plan_trim(P, len1, len2, trim_action, cut1, cut2, m1, m2);
    if (trim_action == 2) {                                            // mask: keep the length, remember the cut
        uend1[r] = a1 + cut1;
        uend2[r] = a2 + cut2;
    } else {
        end1[r] = a1 + cut1;
        end2[r] = a2 + cut2;
    }
    matched1[r] = m1 ? 1 : 0;
    matched2[r] = m2 ? 1 : 0;
}

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

__global__ void emit_total_kernel(const uint32_t *__restrict__ sizes, long long *__restrict__ offsets, long long n) {
    offsets[n] = n ? offsets[n - 1] + (long long)sizes[n - 1] : 0;
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
constexpr int EMIT_STAGE = 13 * 1024;                        // per stage; 2 stages per wave -> 6 waves per CU
// records per wave: 16; full-size stages for records of more than ~400 bytes, half-size stages (twice
// the waves per CU: the kernel is latency bound) for short-read files; 32 records per wave with full
// stages when the caller gives no hint

// LDS -> LDS copy of len bytes at arbitrary alignments: byte steps until dst is dword
// aligned, then one aligned ds_read_b32 + v_alignbyte_b32 + ds_write_b32 per 4 bytes (four
// dwords per batch so that the reads of a batch are in flight together), byte steps for the
// tail.  May read up to 3 bytes beyond src + len (the stages are padded).
__device__ __forceinline__ void lds_copy(uint8_t *dst, const uint8_t *src, uint32_t len) {
    uint32_t k = 0;
    const uint32_t head = min(len, (4u - ((uint32_t)(uintptr_t)dst & 3u)) & 3u);
    for (; k < head; ++k) dst[k] = src[k];
    const uint32_t sm = (uint32_t)(uintptr_t)(src + k) & 3u;
    const uint32_t *sp = (const uint32_t *)(src + k - sm);        // aligned dwords holding the source
    uint32_t *dp = (uint32_t *)(dst + k);
    const uint32_t nd = (len - k) >> 2;
    uint32_t prev = nd ? sp[0] : 0u, t = 0;
    for (; t + 4 <= nd; t += 4) {
        const uint32_t n1 = sp[t + 1], n2 = sp[t + 2], n3 = sp[t + 3], n4 = sp[t + 4];
        dp[t] = __builtin_amdgcn_alignbyte(n1, prev, sm);
        dp[t + 1] = __builtin_amdgcn_alignbyte(n2, n1, sm);
        dp[t + 2] = __builtin_amdgcn_alignbyte(n3, n2, sm);
        dp[t + 3] = __builtin_amdgcn_alignbyte(n4, n3, sm);
        prev = n4;
    }
    for (; t < nd; ++t) {
        const uint32_t nx = sp[t + 1];
        dp[t] = __builtin_amdgcn_alignbyte(nx, prev, sm);
        prev = nx;
    }
    for (k += nd * 4u; k < len; ++k) dst[k] = src[k];
}

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
//            launch_scan           exclusive 64-bit scan of that matrix, group-major: entry (g, b) becomes the
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

// ------------------------------------------------------------------------- MergeOverlapping
__global__ __launch_bounds__(256) void merge_plan_kernel(const int16_t *__restrict__ align, const int32_t *__restrict__ need,
                                                         const FastqRecord *__restrict__ records1,
                                                         const int32_t *__restrict__ begin1, const int32_t *__restrict__ end1,
                                                         const int32_t *__restrict__ begin2, const int32_t *__restrict__ end2,
                                                         long long n, uint8_t *__restrict__ kind, uint32_t *__restrict__ sizes,
                                                         unsigned long long *__restrict__ error) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int len1 = max(0, end1[r] - begin1[r]), len2 = max(0, end2[r] - begin2[r]);
    const MergeShape m = merge_shape(align + 8 * r, len1, len2, need[r]);
    kind[r] = (uint8_t)m.kind;
    uint32_t s = 0;
    if (m.kind == MERGE_INVALID) atomicMin(error, (unsigned long long)r * 8ull + 4ull);
    else if (m.kind != MERGE_NONE) s = fastq_record_bytes(records1[r], m.len[0] + m.len[1]);
    sizes[r] = s;
}

// One wave writes the merged records of 64 consecutive pairs, one after the other (merge_emit_one).
__global__ __launch_bounds__(256) void merge_emit_kernel(const int16_t *__restrict__ align, const uint8_t *__restrict__ kind,
                                                         const uint8_t *__restrict__ bytes1,
                                                         const FastqRecord *__restrict__ records1,
                                                         const uint8_t *__restrict__ bytes2,
                                                         const FastqRecord *__restrict__ records2,
                                                         const int32_t *__restrict__ begin1, const int32_t *__restrict__ end1,
                                                         const int32_t *__restrict__ begin2, const int32_t *__restrict__ end2,
                                                         long long n, const CompTable256 ct, int mate_pass,
                                                         const long long *__restrict__ offsets, uint8_t *__restrict__ out) {
    __shared__ uint8_t s_comp[256];
    s_comp[threadIdx.x] = ct.c[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long r0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (r0 >= n) return;
    const int cnt = (int)min<long long>(64, n - r0);
    for (int i = 0; i < cnt; ++i) {
        const long long r = r0 + i;                               // wave-uniform
        const int k = kind[r];
        if (k == MERGE_NONE || k == MERGE_INVALID) continue;
        const int a1 = begin1[r], a2 = begin2[r];
        const int len1 = max(0, end1[r] - a1), len2 = max(0, end2[r] - a2);
        const MergeShape m = merge_shape(align + 8 * r, len1, len2, 0);
        merge_emit_one(out + offsets[r], m, records1[r], bytes1, a1, records2[r], bytes2, a2, len2, s_comp, mate_pass != 0,
                       lane, 64);
    }
}

// ErrorCorrectorMixin.correct_errors(read1, read2, alignment) of the pairs MergeOverlapping corrects
// (:900-902: a mismatch action is set, the alignment has errors, the insert aligner has not seen the pair).
__global__ __launch_bounds__(256) void merge_correct_kernel(const int16_t *__restrict__ align, const uint8_t *__restrict__ kind,
                                                            const uint8_t *__restrict__ insert_matched, uint8_t *bytes1,
                                                            const FastqRecord *__restrict__ records1, uint8_t *bytes2,
                                                            const FastqRecord *__restrict__ records2,
                                                            const int32_t *__restrict__ begin1, const int32_t *__restrict__ end1,
                                                            const int32_t *__restrict__ begin2, const int32_t *__restrict__ end2,
                                                            long long n, int action, int min_qual_diff, const CompTable256 ct,
                                                            int32_t *__restrict__ corrected,
                                                            unsigned long long *__restrict__ error) {
    __shared__ uint8_t s_comp[256];
    s_comp[threadIdx.x] = ct.c[threadIdx.x];
    __syncthreads();
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    if (corrected) corrected[2 * r] = corrected[2 * r + 1] = 0;
    const int k = kind[r];
    if (k == MERGE_NONE || k == MERGE_INVALID || align[8 * r + 5] <= 0 || (insert_matched && insert_matched[r])) return;
    const FastqRecord r1 = records1[r], r2 = records2[r];
    const int a1 = begin1[r], a2 = begin2[r];
    const int len1 = max(0, end1[r] - a1), len2 = max(0, end2[r] - a2);
    int32_t changed[2], newlen[2];
    correct_errors_one(bytes1 + r1.seq_off + a1, bytes1 + r1.qual_off + a1, len1, bytes2 + r2.seq_off + a2,
                       bytes2 + r2.qual_off + a2, len2, align + 8 * r, action, min_qual_diff, false, s_comp, changed, newlen);
    if (changed[0] < 0) atomicMin(error, (unsigned long long)r * 8ull + (unsigned long long)(-changed[0]));
    else if (corrected) { corrected[2 * r] = changed[0]; corrected[2 * r + 1] = changed[1]; }
}

// ---- pair formatter ---------------------------------------------------------------------
// atr_fastq_emit_pairs: read 1's record, then read 2's, pair after pair (the reference's InterleavedFormatter,
// io/seqio.py:740-749).  The two reads' descriptors index two chunks, or one (an interleaved input).
__global__ __launch_bounds__(256) void emit_pairs_sizes_kernel(const FastqRecord *__restrict__ records1,
                                                               const int32_t *__restrict__ begin1, const int32_t *__restrict__ end1,
                                                               const FastqRecord *__restrict__ records2,
                                                               const int32_t *__restrict__ begin2, const int32_t *__restrict__ end2,
                                                               const uint8_t *__restrict__ dest, int which, long long n,
                                                               uint32_t *__restrict__ sizes) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    uint32_t s = 0;
    if (!dest || dest[r] == which)
        s = pair_text_bytes(mate_text(nullptr, records1, begin1, end1, nullptr, nullptr, r),
                            mate_text(nullptr, records2, begin2, end2, nullptr, nullptr, r));
    sizes[r] = s;
}

// 16-byte blocks global -> LDS, the wave's 64 lanes side by side; src and dst 16-byte aligned
__device__ __forceinline__ void stage_span(uint8_t *dst, const uint8_t *src, uint32_t need, int lane) {
    for (uint32_t o = (uint32_t)lane * 16u; o < need; o += 64u * 16u) *(uint4 *)(dst + o) = *(const uint4 *)(src + o);
}

// One wave formats a tile of TILE consecutive pairs through LDS, as emit_staged_kernel does for TILE records:
//   1. the input spans of the tile -- read 1's records and read 2's, each first '@' .. end of the last quality line --
//      go to LDS with coalesced 16-byte loads: as ONE span when both reads sit in one chunk and the union of the two
//      fits (interleaved input: the two spans are the same bytes but for a record at either end), else side by side;
//   2. four lanes assemble a pair inside an LDS image of the tile's output span: read 1's "@name\nSEQ\n", its
//      "+[name]\nQUAL\n", then the same two of read 2 behind them;
//   3. the image is written with 16-byte stores aligned to the output ADDRESS, the ragged ends with byte stores.
// The alignments are those of the addresses, not of the offsets: a chunk or an output that does not start on a
// 16-byte boundary is staged all the same (the 16-byte block around a span's first and last byte belongs to the
// chunk's allocation and its padding).  STAGE bounds the input stage and the output image each.  A tile with a
// record out of file order or with a rewritten name, or one beyond the stage, is formatted a byte per lane from
// global memory (pair_format).
template <int TILE, int STAGE>
__global__ __launch_bounds__(64) void emit_pairs_staged_kernel(const uint8_t *bytes1, const FastqRecord *__restrict__ records1,
                                                               const int32_t *__restrict__ begin1, const int32_t *__restrict__ end1,
                                                               const int32_t *__restrict__ ubegin1, const int32_t *__restrict__ uend1,
                                                               const uint8_t *bytes2, const FastqRecord *__restrict__ records2,
                                                               const int32_t *__restrict__ begin2, const int32_t *__restrict__ end2,
                                                               const int32_t *__restrict__ ubegin2, const int32_t *__restrict__ uend2,
                                                               const uint8_t *__restrict__ dest, int which, long long n,
                                                               const long long *__restrict__ offsets, uint8_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_pairs[];
    static_assert(64 % TILE == 0 && 64 / TILE >= 4 && STAGE % 16 == 0, "four working lanes per pair, 16-byte stages");
    uint8_t *s_in = s_pairs, *s_out = s_pairs + STAGE;
    constexpr int LPP = 64 / TILE;                            // lanes per pair (the first four do the work)
    const int lane = threadIdx.x, slot = lane / LPP, part = lane % LPP;
    const int mate = (part >> 1) & 1;                         // lanes 0, 1 of a pair: read 1; lanes 2, 3: read 2
    const long long r0 = (long long)blockIdx.x * TILE;
    const int cnt = (int)min<long long>(TILE, n - r0);
    const long long r = r0 + slot;
    const bool live = slot < cnt;
    MateText m = {nullptr, {0, 0, 0, 0, 0, 0, 0, 0}, 0, 0, 0, 0};
    long long off = 0;
    bool keep = false;
    if (live) {
        m = mate ? mate_text(bytes2, records2, begin2, end2, ubegin2, uend2, r)
                 : mate_text(bytes1, records1, begin1, end1, ubegin1, uend1, r);
        off = offsets[r];
        keep = !dest || dest[r] == which;
    }
    const uint32_t size1 = __shfl(mate_text_bytes(m), slot * LPP, 64);             // read 1's text comes first
    const uint32_t rec_lo = m.rec.name_off - 1u, rec_hi = m.rec.qual_off + m.rec.qual_len;
    const uint32_t lo1 = __shfl(rec_lo, 0, 64), hi1 = __shfl(rec_hi, LPP * (cnt - 1), 64);
    const uint32_t lo2 = __shfl(rec_lo, 2, 64), hi2 = __shfl(rec_hi, LPP * (cnt - 1) + 2, 64);
    const long long out_lo = offsets[r0], out_hi = offsets[r0 + cnt];
    if (out_hi == out_lo) return;
    const bool ordered = __all(!live || mate_stageable(m, mate ? lo2 : lo1, mate ? hi2 : hi1));
    // where the spans go: s_in[at_k + (x - lo_k)] = bytes_k[x]
    const uint32_t mis1 = (uint32_t)((uintptr_t)(bytes1 + lo1) & 15u), mis2 = (uint32_t)((uintptr_t)(bytes2 + lo2) & 15u);
    const uint32_t ulo = min(lo1, lo2), uhi = max(hi1, hi2), umis = (uint32_t)((uintptr_t)(bytes1 + ulo) & 15u);
    const bool one = bytes1 == bytes2 && (unsigned long long)(uhi - ulo) + umis + 16ull <= (unsigned long long)STAGE;
    const unsigned long long side2 = ((unsigned long long)mis1 + (hi1 - lo1) + 15ull) & ~15ull;
    const unsigned long long need_in = one ? (unsigned long long)(uhi - ulo) + umis : side2 + mis2 + (hi2 - lo2);
    const uint32_t mis_out = (uint32_t)((uintptr_t)(out + out_lo) & 15u);
    const bool fits = ordered && need_in + 16ull <= (unsigned long long)STAGE &&
                      (unsigned long long)(out_hi - out_lo) + mis_out + 16ull <= (unsigned long long)STAGE;
    if (!fits) {                                           // slow path: a byte per lane straight from / to global
        // (one record per step, read 1's and read 2's in turn: pair_format with one copy of the record code)
        for (int k = 0; k < 2 * cnt; ++k) {
            const long long ri = r0 + (k >> 1);                   // wave-uniform, as is `second`
            const bool second = (k & 1) != 0;
            if (dest && dest[ri] != which) continue;
            const uint32_t before = second ? mate_text_bytes(mate_text(bytes1, records1, begin1, end1, nullptr, nullptr, ri)) : 0u;
            const MateText t = mate_text(second ? bytes2 : bytes1, second ? records2 : records1, second ? begin2 : begin1,
                                         second ? end2 : end1, second ? ubegin2 : ubegin1, second ? uend2 : uend1, ri);
            // (the lane count as the launch gives it, 64: as a literal the copy loops of the record code are
            // unrolled and this rare path doubles the kernel's VGPRs, 88 against 44)
            pair_format_mate(out + offsets[ri], t, before, lane, (int)blockDim.x);
        }
        return;
    }
    // 1. stage the input
    uint32_t at1, at2;
    if (one) {
        at1 = umis + (lo1 - ulo);
        at2 = umis + (lo2 - ulo);
        stage_span(s_in, bytes1 + ulo - umis, (uhi - ulo) + umis, lane);
    } else {
        at1 = mis1;
        at2 = (uint32_t)side2 + mis2;
        stage_span(s_in, bytes1 + lo1 - mis1, mis1 + (hi1 - lo1), lane);
        stage_span(s_in + (uint32_t)side2, bytes2 + lo2 - mis2, mis2 + (hi2 - lo2), lane);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // 2. four lanes format one pair inside the output image
    if (keep && part < 4) {
        const uint8_t *in = s_in + (mate ? at2 : at1);       // in[x - lo] = bytes[x]
        const uint32_t lo = mate ? lo2 : lo1;
        const FastqRecord &rec = m.rec;
        uint8_t *o = s_out + mis_out + (uint32_t)(off - out_lo) + (mate ? size1 : 0u);
        const uint32_t kept = (uint32_t)(m.b - m.a);
        // even lane: '@' name '\n' bases '\n'; odd lane, behind that: '+' [name2] '\n' qualities '\n' -- one
        // instruction stream for both (flag bit 1 is not staged: name2 is the name itself)
        const bool head = !(part & 1);
        const uint32_t len_a = head ? rec.name_len : fastq_name2_len(rec);
        const uint8_t *src_a = in + ((head ? rec.name_off : fastq_name2_off(rec)) - lo);
        const uint8_t *line = in + ((head ? rec.seq_off : rec.qual_off) - lo);
        if (!head) o += 1u + rec.name_len + 1u + kept + 1u;
        *o++ = head ? '@' : '+';
        lds_copy(o, src_a, len_a);
        o += len_a;
        *o++ = '\n';
        if (head && (m.ub > m.a || m.ue < m.b)) {
            for (uint32_t k = 0; k < kept; ++k) o[k] = masked_base(line, m.a + (int)k, m.ub, m.ue);
        } else {
            lds_copy(o, line + m.a, kept);
        }
        o[kept] = '\n';
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // 3. write the image: aligned 16-byte blocks, byte stores at the ragged ends
    {
        uint8_t *dst_al = out + (out_lo - mis_out);
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

// ---- OverwriteRead (op-order W): plan and apply ------------------------------------------------
// plan: a lane per pair sums the window of both reads' kept qualities (overwrite_which) and sizes the clone.
__global__ __launch_bounds__(256) void overwrite_plan_kernel(const uint8_t *bytes1, const FastqRecord *__restrict__ records1,
                                                             const int32_t *__restrict__ begin1, const int32_t *__restrict__ end1,
                                                             const uint8_t *bytes2, const FastqRecord *__restrict__ records2,
                                                             const int32_t *__restrict__ begin2, const int32_t *__restrict__ end2,
                                                             long long n, int lowq, int highq, int window, int base,
                                                             uint8_t *__restrict__ which, uint32_t *__restrict__ sizes1,
                                                             uint32_t *__restrict__ sizes2) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const MateText m1 = mate_text(bytes1, records1, begin1, end1, nullptr, nullptr, r);
    const MateText m2 = mate_text(bytes2, records2, begin2, end2, nullptr, nullptr, r);
    const int len1 = m1.b - m1.a, len2 = m2.b - m2.a;
    const int w = overwrite_which(bytes1 + m1.rec.qual_off + m1.a, len1, bytes2 + m2.rec.qual_off + m2.a, len2, base, lowq,
                                  highq, window);
    which[r] = (uint8_t)w;
    sizes1[r] = w == 1 ? overwrite_clone_bytes(m2.rec, len2) : 0u;
    sizes2[r] = w == 2 ? overwrite_clone_bytes(m1.rec, len1) : 0u;
}

// apply: one wave writes the clones of 64 consecutive pairs, one after the other, into the tails of the grown
// chunks (lanes write forward, read backward), then re-points the overwritten read's descriptor and interval.
__global__ __launch_bounds__(256) void overwrite_apply_kernel(uint8_t *bytes1, FastqRecord *records1, int32_t *begin1,
                                                              int32_t *end1, uint8_t *bytes2, FastqRecord *records2,
                                                              int32_t *begin2, int32_t *end2, long long n,
                                                              const uint8_t *__restrict__ which,
                                                              const long long *__restrict__ grow1,
                                                              const long long *__restrict__ grow2, long long tail1,
                                                              long long tail2, const CompTable256 ct,
                                                              unsigned long long *__restrict__ error) {
    __shared__ uint8_t s_comp[256];
    s_comp[threadIdx.x] = ct.c[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long r0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (r0 >= n) return;
    const int cnt = (int)min<long long>(64, n - r0);
    for (int i = 0; i < cnt; ++i) {
        const long long r = r0 + i;                               // wave-uniform, as is w
        const int w = which[r];
        if (!w) continue;
        const MateText src = w == 1 ? mate_text(bytes2, records2, begin2, end2, nullptr, nullptr, r)
                                    : mate_text(bytes1, records1, begin1, end1, nullptr, nullptr, r);
        const uint32_t at = (uint32_t)(w == 1 ? tail1 + grow1[r] : tail2 + grow2[r]);
        const bool ok = overwrite_clone_write((w == 1 ? bytes1 : bytes2) + at, src, s_comp, lane, 64);
        const bool all_ok = __all(ok);
        if (lane == 0) {
            if (!all_ok) atomicMin(error, (unsigned long long)r * 8ull + 1ull);
            const int kept = src.b - src.a;
            (w == 1 ? records1 : records2)[r] = overwrite_clone_record(src.rec, kept, at);
            (w == 1 ? begin1 : begin2)[r] = 0;
            (w == 1 ? end1 : end2)[r] = kept;
        }
    }
}

static long long scan_blocks(long long n) { return (n + SCAN_BLOCK - 1) / SCAN_BLOCK; }

// exclusive prefix sums of v[n] -> out[n] (int64); `sums` holds scan_blocks(n) uint64
static void launch_scan(const uint32_t *v, long long n, long long *out, unsigned long long *sums, long long *total,
                        hipStream_t st) {
    const long long nb = scan_blocks(n);
    if (n == 0) { if (total) hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, total, 0ll); return; }
    hipLaunchKernelGGL(scan_local_kernel, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, v, n, out, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_BLOCK), 0, st, sums, nb, total);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, out, n, sums, nb);
}

}  // namespace atr

using namespace atr;

static inline unsigned grid256(long long n) { return (unsigned)((n + 255) / 256); }
static inline int launched(const char *what) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ATR_OK : hip_fail(e, what);
}
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" {

// work layout: [block_counts u32 x nblk][block_base i64 x (nblk + 1)][sums u64 x scan_blocks(nblk)][has_cr u32]
size_t atr_fastq_work_bytes(int64_t nbytes) {
    if (nbytes < 0) return 0;
    const long long nblk = (nbytes + NL_BLOCK_BYTES - 1) / NL_BLOCK_BYTES;
    return align256((size_t)nblk * 4) + align256((size_t)(nblk + 1) * 8) + align256((size_t)scan_blocks(nblk) * 8) + 256;
}

int atr_fastq_count_lines(const uint8_t *d_bytes, int64_t nbytes, void *d_work, int64_t *d_nlines, void *stream) {
    if (nbytes < 0 || nbytes >= (int64_t)0xFFFFFFF0ll || !d_nlines) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (nbytes == 0) {
        hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_nlines, 0ll);
        return launched("fastq count launch");
    }
    if (!d_bytes || !d_work || ((uintptr_t)d_bytes & 15)) return ATR_ERR_INVALID;
    const long long nblk = (nbytes + NL_BLOCK_BYTES - 1) / NL_BLOCK_BYTES;
    uint32_t *counts = (uint32_t *)d_work;
    long long *base = (long long *)((char *)d_work + align256((size_t)nblk * 4));
    unsigned long long *sums = (unsigned long long *)((char *)base + align256((size_t)(nblk + 1) * 8));
    uint32_t *has_cr = (uint32_t *)((char *)sums + align256((size_t)scan_blocks(nblk) * 8));
    hipError_t me = hipMemsetAsync(has_cr, 0, 4, st);
    if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync");
    hipLaunchKernelGGL(count_newlines_kernel, dim3((unsigned)nblk), dim3(NL_THREADS), 0, st, d_bytes, (long long)nbytes, counts, has_cr);
    launch_scan(counts, nblk, base, sums, (long long *)d_nlines, st);
    return launched("fastq count launch");
}

int atr_fastq_index(const uint8_t *d_bytes, int64_t nbytes, const void *d_work, uint32_t *d_line_ends, int64_t nlines,
                    atr_fastq_record *d_records, int64_t *d_error, void *stream) {
    if (nbytes < 0 || nbytes >= (int64_t)0xFFFFFFF0ll || nlines < 0 || !d_error) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_error, (long long)LLONG_MAX);
    if (nlines == 0 || nbytes == 0) return launched("fastq index launch");
    if (!d_bytes || !d_work || !d_line_ends || ((uintptr_t)d_bytes & 15)) return ATR_ERR_INVALID;
    const long long nblk = (nbytes + NL_BLOCK_BYTES - 1) / NL_BLOCK_BYTES;
    const long long *base = (const long long *)((const char *)d_work + align256((size_t)nblk * 4));
    const uint32_t *has_cr = (const uint32_t *)((const char *)base + align256((size_t)(nblk + 1) * 8) +
                                                align256((size_t)scan_blocks(nblk) * 8));
    hipLaunchKernelGGL(line_ends_kernel, dim3((unsigned)nblk), dim3(NL_THREADS), 0, st, d_bytes, (long long)nbytes, base, d_line_ends);
    const long long nrec = nlines / 4;
    if (nrec > 0) {
        if (!d_records) return ATR_ERR_INVALID;
        hipLaunchKernelGGL(records_kernel, dim3(grid256(nrec)), dim3(256), 0, st, d_bytes, d_line_ends, nrec, has_cr,
                           (FastqRecord *)d_records, (unsigned long long *)d_error);
    }
    return launched("fastq index launch");
}

int atr_pack_records(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                     const int32_t *d_end, int64_t nreads, int max_len, const uint8_t table[256], int planes,
                     uint8_t *d_packed, int32_t *d_lens, int32_t *d_invalid, void *stream) {
    if (nreads < 0 || max_len < 0 || max_len > ATR_MAX_READ_LEN || !table) return ATR_ERR_INVALID;
    if (nreads == 0) return ATR_OK;
    if (!d_bytes || !d_records || (max_len > 0 && !d_packed) || ((uintptr_t)d_bytes & 15)) return ATR_ERR_INVALID;
    PackTable256 tab;
    memcpy(tab.t, table, 256);
    const int nchunks = (max_len + 31) / 32;
    const long long ntiles = (nreads + 63) / 64;
    const int stride_dw = ((max_len + 6) / 4) | 1;              // dwords per LDS row (odd)
    const size_t per_wave = (size_t)64 * stride_dw * 4;
    const int waves = per_wave * 4 <= 65536 - 256 ? 4 : (per_wave * 2 <= 65536 - 256 ? 2 : 1);
    if (planes)
        hipLaunchKernelGGL(pack_records_kernel<true>, dim3((unsigned)((ntiles + waves - 1) / waves)), dim3(64 * waves),
                           per_wave * waves, (hipStream_t)stream, d_bytes, (const FastqRecord *)d_records, d_begin, d_end,
                           (long long)nreads, max_len, nchunks, stride_dw, tab, (uint4 *)d_packed, d_lens, d_invalid);
    else
        hipLaunchKernelGGL(pack_records_kernel<false>, dim3((unsigned)((ntiles + waves - 1) / waves)), dim3(64 * waves),
                           per_wave * waves, (hipStream_t)stream, d_bytes, (const FastqRecord *)d_records, d_begin, d_end,
                           (long long)nreads, max_len, nchunks, stride_dw, tab, (uint4 *)d_packed, d_lens, d_invalid);
    return launched("pack_records_kernel launch");
}

int atr_clip_batch(const atr_fastq_record *d_records, int32_t *d_begin, int32_t *d_end, int64_t n, int front,
                   int back, void *stream) {
    if (n < 0 || front < 0 || back > 0) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_begin || !d_end) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(clip_kernel, dim3(grid256(n)), dim3(256), 0, (hipStream_t)stream, (const FastqRecord *)d_records,
                       d_begin, d_end, (long long)n, front, back);
    return launched("clip_kernel launch");
}

int atr_quality_trim_batch(const uint8_t *d_bytes, const atr_fastq_record *d_records, int32_t *d_begin,
                           int32_t *d_end, int64_t n, int cutoff_front, int cutoff_back, int base, int nextseq,
                           void *stream) {
    if (n < 0) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_bytes || !d_records || !d_begin || !d_end || ((uintptr_t)d_bytes & 15)) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(quality_trim_kernel, dim3(grid256(n)), dim3(256), 0, (hipStream_t)stream, d_bytes,
                       (const FastqRecord *)d_records, d_begin, d_end, (long long)n, cutoff_front, cutoff_back, base, nextseq);
    return launched("quality_trim_kernel launch");
}

int atr_nend_trim_batch(const uint8_t *d_bytes, const atr_fastq_record *d_records, int32_t *d_begin,
                        int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end, int64_t n,
                        void *stream) {
    if (n < 0 || ((d_unmasked_begin == nullptr) != (d_unmasked_end == nullptr))) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_bytes || !d_records || !d_begin || !d_end) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(nend_trim_kernel, dim3(grid256(n)), dim3(256), 0, (hipStream_t)stream, d_bytes,
                       (const FastqRecord *)d_records, d_begin, d_end, d_unmasked_begin, d_unmasked_end, (long long)n);
    return launched("nend_trim_kernel launch");
}

int atr_match_trim_batch(const atr_result *d_matches, const uint8_t *d_front, int default_front, int32_t *d_begin,
                         int32_t *d_end, uint8_t *d_active, uint8_t *d_matched, int64_t n, void *stream) {
    if (n < 0) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_matches || !d_begin || !d_end) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(match_trim_kernel, dim3(grid256(n)), dim3(256), 0, (hipStream_t)stream, (const int16_t *)d_matches,
                       d_front, default_front, d_begin, d_end, d_active, d_matched, (long long)n);
    return launched("match_trim_kernel launch");
}

int atr_read_filter_batch(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                          const int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end,
                          const uint8_t *d_matched, int64_t n, int min_len, int max_len, double max_n,
                          int discard_trimmed, int discard_untrimmed, uint8_t *d_dest, uint8_t *d_fail_mask,
                          void *stream) {
    if (n < 0 || ((d_unmasked_begin == nullptr) != (d_unmasked_end == nullptr))) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_bytes || !d_records || !d_begin || !d_end || (!d_dest && !d_fail_mask)) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(read_filter_kernel, dim3(grid256(n)), dim3(256), 0, (hipStream_t)stream, d_bytes,
                       (const FastqRecord *)d_records, d_begin, d_end, d_unmasked_begin, d_unmasked_end, d_matched,
                       (long long)n, min_len, max_len, max_n, discard_trimmed, discard_untrimmed, d_dest, d_fail_mask);
    return launched("read_filter_kernel launch");
}

int atr_pair_filter_batch(const uint8_t *d_fail_mask1, const uint8_t *d_fail_mask2, int64_t n, int min_affected,
                          uint8_t *d_dest, void *stream) {
    if (n < 0 || (min_affected != 1 && min_affected != 2)) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_fail_mask1 || !d_fail_mask2 || !d_dest) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(pair_filter_kernel, dim3(grid256(n)), dim3(256), 0, (hipStream_t)stream, d_fail_mask1, d_fail_mask2,
                       (long long)n, min_affected, d_dest);
    return launched("pair_filter_kernel launch");
}

int atr_insert_plan_batch(const atr_result *d_insert, const atr_result *d_fallback1, const atr_result *d_fallback2,
                          uint8_t *d_bytes1, const atr_fastq_record *d_records1, uint8_t *d_bytes2,
                          const atr_fastq_record *d_records2, int32_t *d_begin1, int32_t *d_end1, int32_t *d_begin2,
                          int32_t *d_end2, int32_t *d_unmasked_end1, int32_t *d_unmasked_end2, int64_t n,
                          int min_insert_len, int symmetric, int trim_action, int correct_action, int min_qual_difference,
                          const uint8_t comp[256], uint8_t *d_matched1, uint8_t *d_matched2, int32_t *d_corrected,
                          int64_t *d_error, void *stream) {
    if (n < 0 || trim_action < 0 || trim_action > 2 || correct_action < -1 || correct_action > 2) return ATR_ERR_INVALID;
    if (correct_action >= 0 && (!d_bytes1 || !d_records1 || !d_bytes2 || !d_records2 || !comp || !d_error))
        return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (d_error) hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_error, (long long)LLONG_MAX);
    if (n == 0) return launched("insert_plan_kernel launch");
    if (!d_insert || !d_fallback1 || !d_fallback2 || !d_begin1 || !d_end1 || !d_begin2 || !d_end2 || !d_matched1 ||
        !d_matched2 || (trim_action == 2 && (!d_unmasked_end1 || !d_unmasked_end2)))
        return ATR_ERR_INVALID;
    CompTable256 ct;
    memset(ct.c, 0, 256);
    if (comp) memcpy(ct.c, comp, 256);
    hipLaunchKernelGGL(insert_plan_kernel, dim3(grid256(n)), dim3(256), 0, st, (const int16_t *)d_insert,
                       (const int16_t *)d_fallback1, (const int16_t *)d_fallback2, d_bytes1,
                       (const FastqRecord *)d_records1, d_bytes2, (const FastqRecord *)d_records2, d_begin1, d_end1,
                       d_begin2, d_end2, d_unmasked_end1, d_unmasked_end2, (long long)n, min_insert_len, symmetric,
                       trim_action, correct_action, min_qual_difference, ct, d_matched1, d_matched2, d_corrected,
                       (unsigned long long *)d_error);
    return launched("insert_plan_kernel launch");
}

// work layout: [sizes u32 x n][sums u64 x scan_blocks(n)]
size_t atr_fastq_emit_work_bytes(int64_t n) {
    if (n < 0) return 0;
    return align256((size_t)n * 4) + align256((size_t)scan_blocks(n) * 8) + 256;
}

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
        uint32_t *sizes = (uint32_t *)d_work;
        unsigned long long *sums = (unsigned long long *)((char *)d_work + align256((size_t)n * 4));
        hipLaunchKernelGGL(emit_sizes_kernel, dim3(grid256(n)), dim3(256), 0, st, (const FastqRecord *)d_records, d_begin,
                           d_end, d_dest, dest, (long long)n, sizes);
        launch_scan(sizes, n, (long long *)d_offsets, sums, nullptr, st);
        hipLaunchKernelGGL(emit_total_kernel, dim3(1), dim3(1), 0, st, sizes, (long long *)d_offsets, (long long)n);
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

// work layout: [hist u32 x n_groups * nb][base i64 x n_groups * nb][sums u64 x scan_blocks(n_groups * nb)],
// nb = blocks of GRP_BLOCK records
size_t atr_fastq_emit_grouped_work_bytes(int64_t n, int n_groups) {
    if (n < 0 || n_groups < 1 || n_groups > ATR_EMIT_MAX_GROUPS) return 0;
    const long long cells = (long long)n_groups * ((n + GRP_BLOCK - 1) / GRP_BLOCK);
    return align256((size_t)cells * 4) + align256((size_t)cells * 8) + align256((size_t)scan_blocks(cells) * 8) + 256;
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
        const long long nb = (n + GRP_BLOCK - 1) / GRP_BLOCK, cells = (long long)n_groups * nb;
        uint32_t *hist = (uint32_t *)d_work;
        long long *base = (long long *)((char *)d_work + align256((size_t)cells * 4));
        unsigned long long *sums = (unsigned long long *)((char *)base + align256((size_t)cells * 8));
        hipLaunchKernelGGL(group_hist_kernel, dim3((unsigned)nb), dim3(GRP_BLOCK), (size_t)n_groups * 4, st, records, d_begin,
                           d_end, d_group, n_groups, (long long)n, nb, hist);
        launch_scan(hist, cells, base, sums, (long long *)d_group_offsets + n_groups, st);
        hipLaunchKernelGGL(group_offsets_kernel, dim3((unsigned)nb), dim3(GRP_BLOCK), (size_t)(GRP_BLOCK / 64) * n_groups * 4, st,
                           records, d_begin, d_end, d_group, n_groups, (long long)n, nb, (const long long *)base,
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

size_t atr_merge_work_bytes(int64_t n) { return atr_fastq_emit_work_bytes(n); }

int atr_merge_plan_batch(const atr_result *d_align, const int32_t *d_need, const atr_fastq_record *d_records1,
                         const int32_t *d_begin1, const int32_t *d_end1, const int32_t *d_begin2, const int32_t *d_end2,
                         int64_t n, uint8_t *d_kind, int64_t *d_offsets, void *d_work, int64_t *d_error, void *stream) {
    if (n < 0 || !d_offsets || !d_error) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_error, LLONG_MAX);
    if (n == 0) {
        hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_offsets, 0ll);
        return launched("merge plan launch");
    }
    if (!d_align || !d_need || !d_records1 || !d_begin1 || !d_end1 || !d_begin2 || !d_end2 || !d_kind || !d_work)
        return ATR_ERR_INVALID;
    uint32_t *sizes = (uint32_t *)d_work;
    unsigned long long *sums = (unsigned long long *)((char *)d_work + align256((size_t)n * 4));
    hipLaunchKernelGGL(merge_plan_kernel, dim3(grid256(n)), dim3(256), 0, st, (const int16_t *)d_align, d_need,
                       (const FastqRecord *)d_records1, d_begin1, d_end1, d_begin2, d_end2, (long long)n, d_kind, sizes,
                       (unsigned long long *)d_error);
    launch_scan(sizes, n, (long long *)d_offsets, sums, nullptr, st);
    hipLaunchKernelGGL(emit_total_kernel, dim3(1), dim3(1), 0, st, sizes, (long long *)d_offsets, (long long)n);
    return launched("merge_plan_kernel launch");
}

int atr_merge_emit_batch(const atr_result *d_align, const uint8_t *d_kind, const uint8_t *d_insert_matched,
                         uint8_t *d_bytes1, const atr_fastq_record *d_records1, uint8_t *d_bytes2,
                         const atr_fastq_record *d_records2, const int32_t *d_begin1, const int32_t *d_end1,
                         const int32_t *d_begin2, const int32_t *d_end2, int64_t n, int correct_action,
                         int min_qual_difference, const uint8_t comp[256], const int64_t *d_offsets, int32_t *d_corrected,
                         int64_t *d_error, uint8_t *d_out, void *stream) {
    if (n < 0 || correct_action < -1 || correct_action > 2 || !comp) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_align || !d_kind || !d_bytes1 || !d_records1 || !d_bytes2 || !d_records2 || !d_begin1 || !d_end1 || !d_begin2 ||
        !d_end2 || !d_offsets || !d_error || !d_out)
        return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    CompTable256 ct;
    memcpy(ct.c, comp, 256);
    const unsigned waves = (unsigned)(((n + 63) / 64 + 3) / 4);
    const FastqRecord *rec1 = (const FastqRecord *)d_records1, *rec2 = (const FastqRecord *)d_records2;
    // the mate's bases first: the reference reverse-complements read 2 before it corrects the pair (:887)
    hipLaunchKernelGGL(merge_emit_kernel, dim3(waves), dim3(256), 0, st, (const int16_t *)d_align, d_kind, d_bytes1, rec1,
                       d_bytes2, rec2, d_begin1, d_end1, d_begin2, d_end2, (long long)n, ct, 1, (const long long *)d_offsets,
                       d_out);
    if (correct_action >= 0)
        hipLaunchKernelGGL(merge_correct_kernel, dim3(grid256(n)), dim3(256), 0, st, (const int16_t *)d_align, d_kind,
                           d_insert_matched, d_bytes1, rec1, d_bytes2, rec2, d_begin1, d_end1, d_begin2, d_end2, (long long)n,
                           correct_action, min_qual_difference, ct, d_corrected, (unsigned long long *)d_error);
    hipLaunchKernelGGL(merge_emit_kernel, dim3(waves), dim3(256), 0, st, (const int16_t *)d_align, d_kind, d_bytes1, rec1,
                       d_bytes2, rec2, d_begin1, d_end1, d_begin2, d_end2, (long long)n, ct, 0, (const long long *)d_offsets,
                       d_out);
    return launched("merge_emit_kernel launch");
}

size_t atr_fastq_emit_pairs_work_bytes(int64_t n) { return atr_fastq_emit_work_bytes(n); }

int atr_fastq_emit_pairs(const uint8_t *d_bytes1, const atr_fastq_record *d_records1, const int32_t *d_begin1,
                         const int32_t *d_end1, const int32_t *d_unmasked_begin1, const int32_t *d_unmasked_end1,
                         const uint8_t *d_bytes2, const atr_fastq_record *d_records2, const int32_t *d_begin2,
                         const int32_t *d_end2, const int32_t *d_unmasked_begin2, const int32_t *d_unmasked_end2,
                         const uint8_t *d_dest, int dest, int64_t n, int pair_bytes_hint, int64_t *d_offsets, void *d_work,
                         uint8_t *d_out, void *stream) {
    if (n < 0 || !d_offsets || ((d_unmasked_begin1 == nullptr) != (d_unmasked_end1 == nullptr)) ||
        ((d_unmasked_begin2 == nullptr) != (d_unmasked_end2 == nullptr)))
        return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (!d_out) hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_offsets, 0ll);
        return launched("fastq emit pairs launch");
    }
    if (!d_bytes1 || !d_records1 || !d_begin1 || !d_end1 || !d_bytes2 || !d_records2 || !d_begin2 || !d_end2 || !d_work)
        return ATR_ERR_INVALID;
    const FastqRecord *rec1 = (const FastqRecord *)d_records1, *rec2 = (const FastqRecord *)d_records2;
    if (!d_out) {
        uint32_t *sizes = (uint32_t *)d_work;
        unsigned long long *sums = (unsigned long long *)((char *)d_work + align256((size_t)n * 4));
        hipLaunchKernelGGL(emit_pairs_sizes_kernel, dim3(grid256(n)), dim3(256), 0, st, rec1, d_begin1, d_end1, rec2, d_begin2,
                           d_end2, d_dest, dest, (long long)n, sizes);
        launch_scan(sizes, n, (long long *)d_offsets, sums, nullptr, st);
        hipLaunchKernelGGL(emit_total_kernel, dim3(1), dim3(1), 0, st, sizes, (long long *)d_offsets, (long long)n);
        return launched("fastq emit pairs sizes launch");
    }
    // the tiles and stages of atr_fastq_emit with two records where it has one: 4 pairs and 2 x 3.25 KB per wave for
    // pairs of up to 760 bytes (24 waves per CU), 8 pairs and 2 x 6.5 KB up to 800, else 8 pairs and 2 x 13 KB
#define ATR_EMIT_PAIRS(TILE, STAGE)                                                                                      \
    hipLaunchKernelGGL((emit_pairs_staged_kernel<TILE, STAGE>), dim3((unsigned)((n + TILE - 1) / TILE)), dim3(64),       \
                       2 * (STAGE), st, d_bytes1, rec1, d_begin1, d_end1, d_unmasked_begin1, d_unmasked_end1, d_bytes2,  \
                       rec2, d_begin2, d_end2, d_unmasked_begin2, d_unmasked_end2, d_dest, dest, (long long)n,           \
                       (const long long *)d_offsets, d_out)
    if (pair_bytes_hint > 0 && pair_bytes_hint <= 760) ATR_EMIT_PAIRS(4, EMIT_STAGE / 4);
    else if (pair_bytes_hint > 0 && pair_bytes_hint <= 800) ATR_EMIT_PAIRS(8, EMIT_STAGE / 2);
    else ATR_EMIT_PAIRS(8, EMIT_STAGE);
#undef ATR_EMIT_PAIRS
    return launched("emit_pairs_staged_kernel launch");
}

// work layout: two of atr_fastq_emit's, one per read
size_t atr_overwrite_work_bytes(int64_t n) { return n < 0 ? 0 : 2 * atr_fastq_emit_work_bytes(n); }

int atr_overwrite_plan_batch(const uint8_t *d_bytes1, const atr_fastq_record *d_records1, const int32_t *d_begin1,
                             const int32_t *d_end1, const uint8_t *d_bytes2, const atr_fastq_record *d_records2,
                             const int32_t *d_begin2, const int32_t *d_end2, int64_t n, int lowq, int highq, int window,
                             int quality_base, uint8_t *d_which, int64_t *d_grow1, int64_t *d_grow2, void *d_work,
                             void *stream) {
    if (n < 0 || window < 1 || lowq > highq || quality_base < 0 || quality_base > 255 || !d_grow1 || !d_grow2)
        return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_grow1, 0ll);
        hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_grow2, 0ll);
        return launched("overwrite plan launch");
    }
    if (!d_bytes1 || !d_records1 || !d_begin1 || !d_end1 || !d_bytes2 || !d_records2 || !d_begin2 || !d_end2 || !d_which ||
        !d_work)
        return ATR_ERR_INVALID;
    const size_t half = atr_fastq_emit_work_bytes(n);
    uint32_t *sizes1 = (uint32_t *)d_work, *sizes2 = (uint32_t *)((char *)d_work + half);
    unsigned long long *sums1 = (unsigned long long *)((char *)sizes1 + align256((size_t)n * 4));
    unsigned long long *sums2 = (unsigned long long *)((char *)sizes2 + align256((size_t)n * 4));
    hipLaunchKernelGGL(overwrite_plan_kernel, dim3(grid256(n)), dim3(256), 0, st, d_bytes1, (const FastqRecord *)d_records1,
                       d_begin1, d_end1, d_bytes2, (const FastqRecord *)d_records2, d_begin2, d_end2, (long long)n, lowq, highq,
                       window, quality_base, d_which, sizes1, sizes2);
    launch_scan(sizes1, n, (long long *)d_grow1, sums1, nullptr, st);
    hipLaunchKernelGGL(emit_total_kernel, dim3(1), dim3(1), 0, st, sizes1, (long long *)d_grow1, (long long)n);
    launch_scan(sizes2, n, (long long *)d_grow2, sums2, nullptr, st);
    hipLaunchKernelGGL(emit_total_kernel, dim3(1), dim3(1), 0, st, sizes2, (long long *)d_grow2, (long long)n);
    return launched("overwrite_plan_kernel launch");
}

int atr_overwrite_apply_batch(uint8_t *d_bytes1, atr_fastq_record *d_records1, int32_t *d_begin1, int32_t *d_end1,
                              uint8_t *d_bytes2, atr_fastq_record *d_records2, int32_t *d_begin2, int32_t *d_end2, int64_t n,
                              const uint8_t *d_which, const int64_t *d_grow1, const int64_t *d_grow2, int64_t tail1,
                              int64_t tail2, const uint8_t comp[256], int64_t *d_error, void *stream) {
    if (n < 0 || !comp || !d_error || tail1 < 0 || tail2 < 0) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_error, (long long)LLONG_MAX);
    if (n == 0) return launched("overwrite apply launch");
    if (!d_bytes1 || !d_records1 || !d_begin1 || !d_end1 || !d_bytes2 || !d_records2 || !d_begin2 || !d_end2 || !d_which ||
        !d_grow1 || !d_grow2)
        return ATR_ERR_INVALID;
    CompTable256 ct;
    memcpy(ct.c, comp, 256);
    const unsigned blocks = (unsigned)(((n + 63) / 64 + 3) / 4);
    hipLaunchKernelGGL(overwrite_apply_kernel, dim3(blocks), dim3(256), 0, st, d_bytes1, (FastqRecord *)d_records1, d_begin1,
                       d_end1, d_bytes2, (FastqRecord *)d_records2, d_begin2, d_end2, (long long)n, d_which,
                       (const long long *)d_grow1, (const long long *)d_grow2, (long long)tail1, (long long)tail2, ct,
                       (unsigned long long *)d_error);
    return launched("overwrite_apply_kernel launch");
}

}  // extern "C"
