// pairtext_kernels.hip -- the pair steps of the device-resident FASTQ batch that write text: MergeOverlapping
// (plan, emit, correct), the pair formatter atr_fastq_emit_pairs and OverwriteRead (plan, apply); see
// include/atropos_hip.h, "device-resident FASTQ batch".  The per-pair code is pairtext_core.hpp and misc_core.hpp.
//
// Byte streaming like fastq_kernels.hip.  Every step sizes its output per pair first, the exclusive scan of
// scan_kernels.hpp places it, and a second launch writes it.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>

#include "atropos_hip.h"
#include "fastq_core.hpp"
#include "misc_core.hpp"
#include "pairtext_core.hpp"

#include "fastq_device.hpp"
#include "launch_util.hpp"
#include "scan_kernels.hpp"

namespace atr {

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

namespace {

// work layout of the overwrite plan: a scan_work per read, each with its 256 spare bytes
struct OverwriteWork {
    ScanWork<uint32_t> r1, r2;
    size_t bytes;
};

OverwriteWork overwrite_work(void *work, long long n) {
    OverwriteWork w;
    Workspace ws(work);
    w.r1 = scan_work<uint32_t>(ws, n);
    ws.take<char>(256);
    w.r2 = scan_work<uint32_t>(ws, n);
    w.bytes = ws.bytes();
    return w;
}

}  // namespace
}  // namespace atr

using namespace atr;

extern "C" {

// work layout: scan_work of uint32 sizes
size_t atr_merge_work_bytes(int64_t n) { return n < 0 ? 0 : scan_work_bytes<uint32_t>(n); }

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
    Workspace ws(d_work);
    const ScanWork<uint32_t> w = scan_work<uint32_t>(ws, n);
    hipLaunchKernelGGL(merge_plan_kernel, dim3(grid256(n)), dim3(256), 0, st, (const int16_t *)d_align, d_need,
                       (const FastqRecord *)d_records1, d_begin1, d_end1, d_begin2, d_end2, (long long)n, d_kind, w.sizes,
                       (unsigned long long *)d_error);
    device_scan(w.sizes, n, (u64 *)d_offsets, w.sums, (u64 *)d_offsets + n, st);
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

size_t atr_fastq_emit_pairs_work_bytes(int64_t n) { return atr_merge_work_bytes(n); }

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
        Workspace ws(d_work);
        const ScanWork<uint32_t> w = scan_work<uint32_t>(ws, n);
        hipLaunchKernelGGL(emit_pairs_sizes_kernel, dim3(grid256(n)), dim3(256), 0, st, rec1, d_begin1, d_end1, rec2, d_begin2,
                           d_end2, d_dest, dest, (long long)n, w.sizes);
        device_scan(w.sizes, n, (u64 *)d_offsets, w.sums, (u64 *)d_offsets + n, st);
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

size_t atr_overwrite_work_bytes(int64_t n) { return n < 0 ? 0 : overwrite_work(nullptr, n).bytes; }

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
    const OverwriteWork w = overwrite_work(d_work, n);
    hipLaunchKernelGGL(overwrite_plan_kernel, dim3(grid256(n)), dim3(256), 0, st, d_bytes1, (const FastqRecord *)d_records1,
                       d_begin1, d_end1, d_bytes2, (const FastqRecord *)d_records2, d_begin2, d_end2, (long long)n, lowq, highq,
                       window, quality_base, d_which, w.r1.sizes, w.r2.sizes);
    device_scan(w.r1.sizes, n, (u64 *)d_grow1, w.r1.sums, (u64 *)d_grow1 + n, st);
    device_scan(w.r2.sizes, n, (u64 *)d_grow2, w.r2.sums, (u64 *)d_grow2 + n, st);
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
