// tail_filter.hpp -- the DP tail of the two-pass pre-pass (band reads + window reads of `order`) for ONE aligner,
// compiled at run time (tail_spec.hip, jit.hpp) and launched ONCE behind piece_scatter_kernel, on the caller's stream,
// in place of the band_kernel || window_kernel pair of launch_fast_dp (side stream, event fork, join).
//
//   * blocks [0, win_blocks) of the grid serve the window bins [BAND_BINS, FILTER_BINS) of `order`: the long, latency-bound
//     tasks start first (and at raised wave priority: they share their SIMDs with band waves from then on);
//   * the blocks behind them serve the band bins [0, BAND_BINS).
//
// Same records as the generic pair: the window blocks run the very lane_step / lane_result of locate_core.hpp, the band
// blocks the same cell word, PRIO tie-break, consider<true> order and row-m-before-last-column rule as band_locate /
// band_locate_last (filter_core.hpp) -- tests/emu/emu_tail_spec.cpp compares the two sweeps on the CPU.  What differs
// is how the rows are issued:
//   - the aligner's m, k, indel cost, insw / delw, klimit, min_overlap, the replicated row codes and thr[] are constant
//     expressions of the generated tail_spec_config.h (atr::tspec): no kernel-argument block, no LocateParams copy;
//   - the row loop goes TAIL_ROWS_UNROLL rows at a time (a multiple of eight: the stream-dword feed sits at a
//     compile-time place of the body, its run-time `(i & 7) == 0` is gone) and fetches the row codes of a body with one
//     scalar load; with ATR_TAIL_ROWS_UNROLL >= m the loop is straight-line code with literal row codes
//     (an experiment switch: the straight-line form of all twelve ND variants is larger than the instruction cache);
//   - a band wave requests `order` / `dref` of the task after next and `tdata` of its next task BEFORE it sweeps the
//     current one: the generic kernel starts every task with that chain of three dependent loads and nothing in flight.
#ifndef ATR_TAIL_FILTER_HPP
#define ATR_TAIL_FILTER_HPP

#ifdef ATR_HOST_EMU
#include "filter_core.hpp"
#else
#include "fast_work.hpp"
#endif

namespace atr {

#ifndef ATR_TAIL_ROWS_UNROLL
#define ATR_TAIL_ROWS_UNROLL 8
#endif
#ifndef ATR_TAIL_WINDOW_UNROLL
#define ATR_TAIL_WINDOW_UNROLL 2
#endif
constexpr int TAIL_ROWS_UNROLL = ATR_TAIL_ROWS_UNROLL;
static_assert(TAIL_ROWS_UNROLL >= 8 && TAIL_ROWS_UNROLL % 8 == 0, "the feed position is a compile-time place of the body");

// one row of the band: cells c = 0 .. ND - 1 in place, exactly band_rows' cell (filter_core.hpp)
template <bool AND_MODE, int ND>
ATR_DEV void tail_band_row(const Uniform &u, uint32_t rrep, uint32_t qw0, uint32_t qw1, uint32_t (&band)[BAND_W]) {
    const uint32_t inf = ((uint32_t)INIT_COST_CAP << CSH) | ORG_BIAS;
    uint32_t m0 = nibble_any(AND_MODE ? (qw0 & rrep) : (qw0 ^ rrep));
    uint32_t m1 = ND > 8 ? nibble_any(AND_MODE ? (qw1 & rrep) : (qw1 ^ rrep)) : 0u;
    if (AND_MODE) { m0 = ~m0; m1 = ~m1; }
    uint32_t left = inf;
#pragma unroll
    for (int c = 0; c < ND; ++c) {
        const uint32_t bit = atr_bfe1(c < 8 ? m0 : m1, 4 * (c & 7) + 3);
        const uint32_t cd = atr_mad24(bit, COST1 + MATCH1, band[c]);
        const uint32_t up = c + 1 < ND ? band[c + 1 < ND ? c + 1 : 0] : inf;
        const uint32_t nw = atr_minu(atr_minu(cd, left + u.delw), up + u.insw) & ~PRIO_MASK;
        band[c] = nw;
        left = nw;
    }
}

// what the rows of a last-column band read are tested with (band_rows_last, filter_core.hpp)
struct TailLast {
    int cap_lo, top, r0, at0, n, cindel;
    bool active;
};

// Rows 1 .. rows of the band, TAIL_ROWS_UNROLL to a body.  LAST: cell (i, n) of the lane's rows of interest goes through
// the candidate test after row i, as in band_rows_last.
// rreps: the replicated row codes, rreps[i - 1] (a constant table of the generated header: scalar loads, or literals
// when the body covers every row).  rows <= ROWS_MAX, a constant expression in the run-time compiled kernel.
template <bool AND_MODE, int ND, int ROWS_MAX, bool LAST>
ATR_DEV void tail_band_sweep(const Uniform &u, const uint32_t *rreps, int rows, const uint32_t *ns, int nss,
                             uint32_t (&band)[BAND_W], const TailLast &tl, const int16_t *thr, Best &best) {
    uint32_t qw0 = ns[0], qw1 = ns[(size_t)nss];
    uint32_t feed = ns[(size_t)2 * nss];
#pragma unroll 1
    for (int i0 = 0; i0 < ROWS_MAX; i0 += TAIL_ROWS_UNROLL) {
        if (i0 >= rows) break;                                     // wave-uniform
#pragma unroll
        for (int t = 0; t < TAIL_ROWS_UNROLL; ++t) {
            const int i = i0 + t + 1;
            if (i <= ROWS_MAX && i <= rows) {                      // wave-uniform
                tail_band_row<AND_MODE, ND>(u, rreps[i - 1], qw0, qw1, band);
                if (LAST && i >= tl.cap_lo) {                      // wave-uniform: some lane's rows of interest have begun
                    const int at = tl.at0 - i;                     // this lane's band index of cell (i, n): n - dlo - i
                    if (tl.active && i <= tl.top && i >= tl.r0 && (u.er || i == u.m)) {
                        uint32_t cell = band[0];
#pragma unroll
                        for (int c = 1; c < ND; ++c) cell = at == c ? band[c] : cell;
                        if (cell < u.klimit) consider<true>(best, cell, i, tl.n, u.min_overlap, thr, tl.cindel);
                    }
                }
                qw0 = (qw0 >> 4) | (qw1 << 28);
                qw1 = (qw1 >> 4) | (feed << 28);
                feed >>= 4;
                if (((t + 1) & 7) == 0) {                          // (i & 7) == 0, at compile time
                    const int k = 2 + (i >> 3);
                    feed = k < BAND_STREAM ? ns[(size_t)k * nss] : 0u;
                }
            }
        }
    }
}

ATR_DEV void tail_band_record(const Best &best, int none_cost, uint32_t rec[4]) {
    const int cost = (int)(best.word >> CSH);
    int refstart = 0, querystart = 0, refstop = -1, querystop = 0, matches = 0, errors = 0;
    if (cost != none_cost) {
        const int origin = (int)(best.word & ORG_MASK) - (int)ORG_BIAS;
        if (origin >= 0) querystart = origin; else refstart = -origin;
        refstop = best.ref_stop; querystop = best.query_stop;
        matches = best.matches; errors = cost;
    }
    rec[0] = (uint32_t)(refstart & 0xFFFF) | ((uint32_t)(refstop & 0xFFFF) << 16);
    rec[1] = (uint32_t)(querystart & 0xFFFF) | ((uint32_t)(querystop & 0xFFFF) << 16);
    rec[2] = (uint32_t)(matches & 0xFFFF) | ((uint32_t)(errors & 0xFFFF) << 16);
    rec[3] = 0;
}

// band_locate (filter_core.hpp) with the sweep above; ROWS_MAX >= u.m
template <bool AND_MODE, int ROWS_MAX>
ATR_DEV void tail_band_locate(const Uniform &u, const uint32_t *rreps, bool noindel, const uint32_t *ns, int nss, int n,
                              uint32_t ww, int smax, const int16_t *thr, uint32_t rec[4]) {
    const int dlo = window_lo(ww);
    uint32_t band[BAND_W];
#pragma unroll
    for (int c = 0; c < BAND_W; ++c) band[c] = ORG_BIAS + (uint32_t)(dlo + c);
    Best best;
    best.key = COST_FIELD_MAX - (u.m + n);
    best.word = (uint32_t)(u.m + n) << CSH;
    best.ref_stop = u.m; best.query_stop = n; best.matches = 0;
    const TailLast none = {0, 0, 0, 0, 0, 0, false};
    if (smax < 8) tail_band_sweep<AND_MODE, 8, ROWS_MAX, false>(u, rreps, u.m, ns, nss, band, none, thr, best);          // wave-uniform
    else if (smax < 10) tail_band_sweep<AND_MODE, 10, ROWS_MAX, false>(u, rreps, u.m, ns, nss, band, none, thr, best);
    else if (smax < 12) tail_band_sweep<AND_MODE, 12, ROWS_MAX, false>(u, rreps, u.m, ns, nss, band, none, thr, best);
    else if (smax < 14) tail_band_sweep<AND_MODE, 14, ROWS_MAX, false>(u, rreps, u.m, ns, nss, band, none, thr, best);
    else tail_band_sweep<AND_MODE, 16, ROWS_MAX, false>(u, rreps, u.m, ns, nss, band, none, thr, best);
    const int cindel = noindel ? 0 : u.indel;
#pragma unroll
    for (int c = 0; c < BAND_W; ++c) {
        const int j = dlo + u.m + c;
        if (c <= smax && band[c] < u.klimit && j <= n) consider<true>(best, band[c], u.m, j, u.min_overlap, thr, cindel);
    }
    tail_band_record(best, u.m + n, rec);
}

// band_locate_last (filter_core.hpp) with the sweep above
template <bool AND_MODE, int ROWS_MAX>
ATR_DEV void tail_band_locate_last(const Uniform &u, const uint32_t *rreps, bool noindel, const uint32_t *ns, int nss, int n,
                                   uint32_t ww, bool active, int smax, int rows_max, int cap_lo, const int16_t *thr,
                                   uint32_t rec[4]) {
    const int dlo = window_lo(ww), top = window_rows(ww), r0 = top - last_band_span(ww), at0 = n - dlo;
    uint32_t band[BAND_W];
#pragma unroll
    for (int c = 0; c < BAND_W; ++c) band[c] = ORG_BIAS + (uint32_t)(dlo + c);
    Best best, bm;                                   // last-column candidates / row-m candidates
    best.key = COST_FIELD_MAX - (u.m + n);
    best.word = (uint32_t)(u.m + n) << CSH;
    best.ref_stop = u.m; best.query_stop = n; best.matches = 0;
    bm = best;
    const int cindel = noindel ? 0 : u.indel;
    const TailLast tl = {cap_lo, top, r0, at0, n, cindel, active};
    if (smax < 4) tail_band_sweep<AND_MODE, 4, ROWS_MAX, true>(u, rreps, rows_max, ns, nss, band, tl, thr, best);
    else if (smax < 6) tail_band_sweep<AND_MODE, 6, ROWS_MAX, true>(u, rreps, rows_max, ns, nss, band, tl, thr, best);
    else if (smax < 8) tail_band_sweep<AND_MODE, 8, ROWS_MAX, true>(u, rreps, rows_max, ns, nss, band, tl, thr, best);
    else if (smax < 10) tail_band_sweep<AND_MODE, 10, ROWS_MAX, true>(u, rreps, rows_max, ns, nss, band, tl, thr, best);
    else if (smax < 12) tail_band_sweep<AND_MODE, 12, ROWS_MAX, true>(u, rreps, rows_max, ns, nss, band, tl, thr, best);
    else if (smax < 14) tail_band_sweep<AND_MODE, 14, ROWS_MAX, true>(u, rreps, rows_max, ns, nss, band, tl, thr, best);
    else tail_band_sweep<AND_MODE, 16, ROWS_MAX, true>(u, rreps, rows_max, ns, nss, band, tl, thr, best);
    if (last_band_rowm(ww) && rows_max == u.m) {
        // the row-m cells of the band, in column order -- the reference sees them BEFORE the last column
        const int width = last_band_width(ww);
#pragma unroll
        for (int c = 0; c < BAND_W; ++c) {
            const int j = dlo + u.m + c;
            if (c <= width && band[c] < u.klimit && j <= n) consider<true>(bm, band[c], u.m, j, u.min_overlap, thr, cindel);
        }
        if (bm.key >= best.key) best = bm;
    }
    tail_band_record(best, u.m + n, rec);
}

#if defined(ATR_TAIL_SPEC) && !defined(ATR_HOST_EMU)
#include "tail_spec_config.h"    // written by the host for this aligner (jit.hpp, tail_config): atr::tspec::*

__device__ __forceinline__ Uniform tail_uniform() {
    Uniform u;
    u.m = tspec::M; u.k = tspec::K; u.p0 = tspec::MT - tspec::M; u.indel = tspec::INDEL; u.min_overlap = tspec::MIN_OVERLAP;
    u.sr = (tspec::FLAGS & ATR_START_WITHIN_SEQ1) != 0; u.sq = (tspec::FLAGS & ATR_START_WITHIN_SEQ2) != 0;
    u.er = (tspec::FLAGS & ATR_STOP_WITHIN_SEQ1) != 0;  u.eq = (tspec::FLAGS & ATR_STOP_WITHIN_SEQ2) != 0;
    u.first_p = u.p0 + (u.er ? 0 : u.m);
    u.insw = (uint32_t)u.indel * COST1 + PRIO_INS;
    u.delw = (uint32_t)u.indel * COST1 + PRIO_DEL;
    u.klimit = (uint32_t)(u.k + 1) << CSH;
    return u;
}

// tasks per wave (locate_fast.hpp, dp_lanes_per_wave)
__device__ __forceinline__ int tail_lanes_per_wave(long long tasks, long long grid_waves, int fixed) {
    if (fixed) return fixed;
    int lpw = 1;
    while (lpw < 64 && (long long)lpw * grid_waves < tasks) lpw <<= 1;
    return lpw;
}

struct TailShared {
    int16_t thr[tspec::M + 2];
    uint32_t init[tspec::MT + 1];
    __attribute__((aligned(16))) uint32_t nm[16][4];
    uint32_t stream[4][BAND_STREAM][64];             // band blocks, per wave: the staged reads, [dword][lane]
    uint32_t spread[4][256];                         // bytes of a plane -> nibbles (piece_core.hpp)
};

// ---- band blocks: band_kernel<AND, false, PLANES> (locate_fast.hpp) over blocks [0, nblocks) -------------------
__device__ __forceinline__ void tail_band_blocks(TailShared &S, int block, int nblocks, const uint4 *__restrict__ packed,
                                                 const int32_t *__restrict__ lens, int nchunks, int max_len,
                                                 uint4 *__restrict__ out, const FastWork &wk) {
    constexpr int M = tspec::M;
    const Uniform u = tail_uniform();
    const long long total = (long long)wk.binbase[BAND_BINS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long stride = (long long)nblocks * 4;
    const int lpw = tail_lanes_per_wave(total, stride, wk.lpw);
    const long long nwaves = (total + lpw - 1) / lpw;
    uint32_t *ns = &S.stream[wave][0][lane];
    long long wv = (long long)block * 4 + wave;
    if (wv >= nwaves) return;
    // the pipeline of a wave: `order` / `dref` of task t + 2 and `tdata` (+ the read length) of task t + 1 are requested
    // before task t is swept
    auto slot_of = [&](long long w) { return w * lpw + lane; };
    auto live_of = [&](long long w) { return w < nwaves && lane < lpw && slot_of(w) < total; };
    auto dense_of = [&](long long w, uint2 task) { return live_of(w) && (task.y & PIECE_NODENSE) == 0u; };
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    uint2 task = live_of(wv) ? wk.order[slot_of(wv)] : make_uint2(0u, 0u);
    uint32_t di = live_of(wv) ? wk.dref[slot_of(wv)] : 0u;
    uint2 task1 = live_of(wv + stride) ? wk.order[slot_of(wv + stride)] : make_uint2(0u, 0u);
    uint32_t di1 = live_of(wv + stride) ? wk.dref[slot_of(wv + stride)] : 0u;
    uint4 a = dense_of(wv, task) ? wk.tdata[2 * (size_t)di] : zero4, b = dense_of(wv, task) ? wk.tdata[2 * (size_t)di + 1] : zero4;
    int n = live_of(wv) ? (lens ? lens[task.x] : max_len) : 0;
    for (; wv < nwaves; wv += stride) {
        const bool live = live_of(wv);
        const long long r = (long long)task.x;
        const uint32_t ww = task.y;
        // the next task's record and length, the task after next
        const bool dense1 = dense_of(wv + stride, task1);
        const uint4 a1 = dense1 ? wk.tdata[2 * (size_t)di1] : zero4, b1 = dense1 ? wk.tdata[2 * (size_t)di1 + 1] : zero4;
        const int n1 = live_of(wv + stride) ? (lens ? lens[task1.x] : max_len) : 0;
        const bool live2 = live_of(wv + 2 * stride);
        const uint2 task2 = live2 ? wk.order[slot_of(wv + 2 * stride)] : make_uint2(0u, 0u);
        const uint32_t di2 = live2 ? wk.dref[slot_of(wv + 2 * stride)] : 0u;

        const bool last = live && window_scan(ww);
        const bool any_last = wave_max_i32(last ? 1 : 0) != 0, any_rowm = wave_max_i32(live && !last ? 1 : 0) != 0;
        const int s_lane = (live && !last) ? window_hi(ww) - u.m + u.k - window_lo(ww) : 0;
        const int smax = min(BAND_W - 1, wave_max_i32(s_lane));
        const bool dense = live && (ww & PIECE_NODENSE) == 0u;
        if (dense) {
            ns[0] = a.x; ns[64] = a.y; ns[128] = a.z; ns[192] = a.w;
            ns[256] = b.x; ns[320] = b.y; ns[384] = b.z; ns[448] = b.w;
        }
        if (wave_max_i32(live && !dense ? 1 : 0) != 0) {           // entries of the full-sweep kernel: gathered from the batch
            const uint32_t *q = (const uint32_t *)(packed + ((size_t)(r >> 6) * nchunks) * 64 + (r & 63));
            if (live && !dense) band_stage_planes(q, nchunks, window_lo(ww), ns, 64, S.spread, band_stream_dwords(M));
        }
        uint32_t rec[4] = {0xFFFF0000u, 0u, 0u, 0u};
        if (any_rowm) tail_band_locate<tspec::AND_MODE, M>(u, tspec::RREP, tspec::NOINDEL, ns, 64, n, ww, smax, S.thr, rec);
        if (any_last) {
            const int smax_l = min(BAND_W - 1, wave_max_i32(last ? last_band_width(ww) : 0));
            const int rows_max = wave_max_i32(last ? (last_band_rowm(ww) ? u.m : window_rows(ww)) : 0);
            const int cap_lo = wave_min_i32(last ? window_rows(ww) - last_band_span(ww) : 0x7fffffff);
            uint32_t rec_l[4];
            tail_band_locate_last<tspec::AND_MODE, M>(u, tspec::RREP, tspec::NOINDEL, ns, 64, n, ww, last, smax_l, min(rows_max, M), cap_lo, S.thr, rec_l);
            if (last) { rec[0] = rec_l[0]; rec[1] = rec_l[1]; rec[2] = rec_l[2]; rec[3] = rec_l[3]; }
        }
        if (live) out[r] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
        task = task1; di = di1; a = a1; b = b1; n = n1;
        task1 = task2; di1 = di2;
    }
}

template <int W>
__device__ __forceinline__ void tail_load_mask(uint32_t (&nm)[W], const uint32_t (*s_nm)[4], uint32_t q) {
#pragma unroll
    for (int w = 0; w < W; ++w) nm[w] = s_nm[q][w];
}

// ---- window blocks: window_kernel<MT, NOINDEL, false, PLANES> (locate_fast.hpp) over blocks [0, nblocks) --------
__device__ __forceinline__ void tail_window_blocks(TailShared &S, int block, int nblocks, const uint4 *__restrict__ packed,
                                                   const int32_t *__restrict__ lens, int nchunks, int max_len,
                                                   uint4 *__restrict__ out, const FastWork &wk) {
    constexpr int MT = tspec::MT;
    constexpr bool NOINDEL = tspec::NOINDEL;
    const Uniform u = tail_uniform();
    const int16_t *s_thr = S.thr;
    const uint32_t *s_init = S.init;
    const uint32_t (*s_nm)[4] = S.nm;
    const uint32_t (*s_spread)[256] = S.spread;
    const long long first = (long long)wk.binbase[BAND_BINS], total = (long long)wk.binbase[FILTER_BINS];
    if (total <= first) return;
    const int lane = threadIdx.x & 63;
    const int lpw = tail_lanes_per_wave(total - first, (long long)nblocks * 4, wk.lpw);
    const long long nwaves = (total - first + lpw - 1) / lpw;
    __builtin_amdgcn_s_setprio(3);                                 // few, long, serial tasks next to the band waves
    for (long long wv = (long long)block * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); wv < nwaves;
         wv += (long long)nblocks * 4) {
        const long long slot = first + wv * lpw + lane;
        const bool live = lane < lpw && slot < total;
        const uint2 task = live ? wk.order[slot] : make_uint2(0u, 0u);
        const long long r = (long long)task.x;
        const uint32_t ww = task.y;
        const int n = live ? (lens ? lens[r] : max_len) : 0;
        const int j_lo = window_lo(ww), j_hi = live ? window_hi(ww) : 0;
        const bool has_window = live && j_hi > j_lo;
        const int jlo = wave_min_i32(live ? j_lo : 0x7fffffff);
        const int jhi = wave_max_i32(has_window ? j_hi : 0);
        const int rows_w = wave_max_i32(live ? window_rows(ww) : 0);
        const int plimit = u.p0 + rows_w;
        const bool head = !(u.sr && jlo == 0);
        const bool rows_wave = __builtin_amdgcn_readfirstlane((int)(first + wv * lpw >= (long long)wk.binbase[ROWS_BIN0])) != 0;
        const bool tri = rows_wave && head && lens == nullptr;

        LaneState<MT> L;
        const uint4 *tp = packed + ((size_t)(r >> 6) * nchunks) * 64 + (r & 63);

        // TAIL MODE (ragged batches, waves of the row-count bins): see window_kernel
        if (lens != nullptr && rows_wave && !u.sr) {
            const int shift = live ? max_len - n : 0;
            const int v0 = wave_min_i32(live ? j_lo + shift : 0x7fffffff);
            if (max_len - v0 <= TAIL_COLUMNS && v0 < max_len) {
                const int s_top_t = wave_max_i32(shift);
                lane_init_window<MT, NOINDEL>(L, u, max_len, v0, live ? max_len : 0, live && window_scan(ww), s_init, s_thr);
                uint32_t tb[TAIL_COLUMNS / 8];
                {
                    const int dlo = n - TAIL_COLUMNS;
                    const int z0 = dlo >> 3;
                    const uint32_t sh = 4u * (uint32_t)(dlo & 7);
                    uint32_t raw[TAIL_COLUMNS / 8 + 1];
#pragma unroll
                    for (int t = 0; t <= TAIL_COLUMNS / 8; ++t)
                        raw[t] = live ? read_dword_planes((const uint32_t *)tp, nchunks, z0 + t, s_spread) : 0u;
#pragma unroll
                    for (int t = 0; t < TAIL_COLUMNS / 8; ++t) tb[t] = sh ? ((raw[t] >> sh) | (raw[t + 1] << (32u - sh))) : raw[t];
                }
                int j = max_len - TAIL_COLUMNS;
#pragma unroll 1
                for (int d = 0; d < TAIL_COLUMNS / 8; ++d) {
                    uint32_t w = tb[0];
#pragma unroll
                    for (int t = 0; t + 1 < TAIL_COLUMNS / 8; ++t) tb[t] = tb[t + 1];
#pragma unroll 1
                    for (int b = 0; b < 8; ++b) {
                        ++j;
                        const uint32_t q = w & 15u;
                        w >>= 4;
                        if (j <= v0) continue;
                        uint32_t nm[(MT + 31) / 32];
                        tail_load_mask(nm, s_nm, q);
                        int pl = min(plimit, u.p0 + (j - v0) + u.k);
                        pl = min(pl, u.p0 + triangle_rows(rows_w, max_len, j, u.k));
                        lane_step<MT, NOINDEL, true, true>(L, u, j, nm, s_thr, pl);
                        if (j <= s_top_t && shift == j) lane_restart_window<MT>(L, u, j);
                    }
                }
                if (live) {
                    uint32_t rec[4];
                    lane_result<MT>(L, u, rec);
                    if ((rec[0] >> 16) != 0xFFFFu) rec[1] -= (uint32_t)shift * 0x00010001u;
                    out[r] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
                }
                continue;
            }
        }
        lane_init_window<MT, NOINDEL>(L, u, n, jlo, j_hi, live && window_scan(ww), s_init, s_thr);
        if (jhi > jlo) {
            const int c0 = jlo >> 5, c1 = (jhi + 31) >> 5;
            uint4 nxt = tp[(size_t)c0 * 64];
            for (int c = c0; c < c1; ++c) {
                uint4 cur = nxt;
                if (c + 1 < c1) nxt = tp[(size_t)(c + 1) * 64];
                cur = make_uint4(piece_nibbles(s_spread, cur.x, cur.y, cur.z, cur.w, 0), piece_nibbles(s_spread, cur.x, cur.y, cur.z, cur.w, 1),
                                 piece_nibbles(s_spread, cur.x, cur.y, cur.z, cur.w, 2), piece_nibbles(s_spread, cur.x, cur.y, cur.z, cur.w, 3));
                int j = c * 32;
#pragma unroll 1
                for (int d = 0; d < 4; ++d) {
                    uint32_t w = cur.x;
                    cur.x = cur.y; cur.y = cur.z; cur.z = cur.w;
                    // (two columns to a body: the next column's mask is fetched from LDS while a column's serial row chain
                    // runs -- the generic kernel keeps one column per body; eight cost 50 kB of code, most of the instruction cache)
#pragma unroll ATR_TAIL_WINDOW_UNROLL
                    for (int b = 0; b < 8; ++b) {
                        ++j;
                        const uint32_t q = w & 15u;
                        w >>= 4;
                        if (j <= jlo || j > jhi) continue;
                        uint32_t nm[(MT + 31) / 32];
                        tail_load_mask(nm, s_nm, q);
                        int pl = head ? min(plimit, u.p0 + (j - jlo) + u.k) : plimit;
                        if (tri) pl = min(pl, u.p0 + triangle_rows(rows_w, max_len, j, u.k));
                        lane_step<MT, NOINDEL, true, true>(L, u, j, nm, s_thr, pl);
                    }
                }
            }
        }
        if (live) {
            uint32_t rec[4];
            lane_result<MT>(L, u, rec);
            out[r] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
        }
    }
}

// the kernel body: win_blocks window blocks, then the band blocks
__device__ __forceinline__ void tail_body(const uint4 *__restrict__ packed, const int32_t *__restrict__ lens, int nchunks,
                                          int max_len, uint4 *__restrict__ out, const FastWork &wk, int win_blocks) {
    __shared__ TailShared S;
    for (int i = threadIdx.x; i <= tspec::MT + 1; i += 256) {
        if (i <= tspec::M + 1) S.thr[i] = tspec::THR[i];
        if (i <= tspec::MT) S.init[i] = init_word(i - (tspec::MT - tspec::M), 0, (tspec::FLAGS & ATR_START_WITHIN_SEQ1) != 0,
                                                  (tspec::FLAGS & ATR_START_WITHIN_SEQ2) != 0, tspec::INDEL);
    }
    if (threadIdx.x < 64) S.nm[threadIdx.x >> 2][threadIdx.x & 3] = tspec::NMASK[threadIdx.x >> 2][threadIdx.x & 3];
    piece_spread_fill(S.spread);
    __syncthreads();
    const int block = (int)blockIdx.x, nblocks = (int)gridDim.x;
    if (block < win_blocks) tail_window_blocks(S, block, win_blocks, packed, lens, nchunks, max_len, out, wk);
    else tail_band_blocks(S, block - win_blocks, nblocks - win_blocks, packed, lens, nchunks, max_len, out, wk);
}
#endif  // ATR_TAIL_SPEC

}  // namespace atr
#endif
