// fastq_kernels.hip -- the device-resident FASTQ batch: line index, record descriptors,
// 4-bit pack straight from the file bytes, interval-update trimmers, filters and the insert
// plan (see include/atropos_hip.h, "device-resident FASTQ batch").  The formatters are
// fastq_emit_kernels.hip, the pair steps that write text pairtext_kernels.hip.
//
// All of this is byte streaming: every kernel is bound by HBM traffic or by the number of
// scattered byte accesses, none has arithmetic worth speaking of.  Layout decisions:
//   * the file chunk stays as it came off the disk; records are 32-byte descriptors
//     (offsets into the chunk), modifier state is two int32 per read;
//   * line ends are found with 16-byte loads + a SWAR zero-byte test, positions come from
//     the exclusive scan of scan_kernels.hpp (no atomics, input order preserved);
//   * the packer copies each sequence line into an LDS row with one direct-to-LDS load
//     (global_load_lds_dword) and lets every lane re-align its row in registers (v_alignbyte_b32).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>

#include "atropos_hip.h"
#include "locate_core.hpp"
#include "fastq_core.hpp"
#include "misc_core.hpp"

#include "pack_fast.hpp"
#include "fastq_device.hpp"
#include "launch_util.hpp"
#include "scan_kernels.hpp"

namespace atr {

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

namespace {

// work layout: [block_counts u32 x nblk][block_base u64 x (nblk + 1)][sums u64 x scan_blocks(nblk)][has_cr u32]
struct IndexWork {
    uint32_t *counts, *has_cr;
    u64 *base, *sums;
    long long nblk;
    size_t bytes;
};

inline IndexWork index_work(const void *work, long long nbytes) {
    IndexWork w;
    Workspace ws(work);
    w.nblk = blocks(nbytes, NL_BLOCK_BYTES);
    w.counts = ws.take<uint32_t>((size_t)w.nblk);
    w.base = ws.take<u64>((size_t)w.nblk + 1);
    w.sums = ws.take<u64>((size_t)scan_blocks(w.nblk));
    w.bytes = ws.bytes();
    w.has_cr = ws.take<uint32_t>(1);                          // (the one word lives in the spare bytes)
    return w;
}

}  // namespace
}  // namespace atr

using namespace atr;

extern "C" {

size_t atr_fastq_work_bytes(int64_t nbytes) { return nbytes < 0 ? 0 : index_work(nullptr, nbytes).bytes; }

int atr_fastq_count_lines(const uint8_t *d_bytes, int64_t nbytes, void *d_work, int64_t *d_nlines, void *stream) {
    if (nbytes < 0 || nbytes >= (int64_t)0xFFFFFFF0ll || !d_nlines) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (nbytes == 0) {
        hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_nlines, 0ll);
        return launched("fastq count launch");
    }
    if (!d_bytes || !d_work || ((uintptr_t)d_bytes & 15)) return ATR_ERR_INVALID;
    const IndexWork w = index_work(d_work, nbytes);
    hipError_t me = hipMemsetAsync(w.has_cr, 0, 4, st);
    if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync");
    hipLaunchKernelGGL(count_newlines_kernel, dim3((unsigned)w.nblk), dim3(NL_THREADS), 0, st, d_bytes, (long long)nbytes,
                       w.counts, w.has_cr);
    device_scan(w.counts, w.nblk, w.base, w.sums, (u64 *)d_nlines, st);
    return launched("fastq count launch");
}

int atr_fastq_index(const uint8_t *d_bytes, int64_t nbytes, const void *d_work, uint32_t *d_line_ends, int64_t nlines,
                    atr_fastq_record *d_records, int64_t *d_error, void *stream) {
    if (nbytes < 0 || nbytes >= (int64_t)0xFFFFFFF0ll || nlines < 0 || !d_error) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_error, (long long)LLONG_MAX);
    if (nlines == 0 || nbytes == 0) return launched("fastq index launch");
    if (!d_bytes || !d_work || !d_line_ends || ((uintptr_t)d_bytes & 15)) return ATR_ERR_INVALID;
    const IndexWork w = index_work(d_work, nbytes);
    hipLaunchKernelGGL(line_ends_kernel, dim3((unsigned)w.nblk), dim3(NL_THREADS), 0, st, d_bytes, (long long)nbytes,
                       (const long long *)w.base, d_line_ends);
    const long long nrec = nlines / 4;
    if (nrec > 0) {
        if (!d_records) return ATR_ERR_INVALID;
        hipLaunchKernelGGL(records_kernel, dim3(grid256(nrec)), dim3(256), 0, st, d_bytes, d_line_ends, nrec,
                           (const uint32_t *)w.has_cr, (FastqRecord *)d_records, (unsigned long long *)d_error);
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

}  // extern "C"
