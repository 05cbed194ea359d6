// stats_core.hpp -- layout of the read-statistics block and the integer forms of the reference's
// per-read rounding (ReadStatistics.collect_record, commands/stats.py:194-255).  Shared by the
// kernels (stats_kernels.hip) and their host entry points.
#pragma once
#include <stdint.h>

#ifndef ATR_HD
#define ATR_HD __host__ __device__ __forceinline__
#endif

namespace atr {

// The block is an array of uint64 counters; for a capacity of L positions:
//   [0, ST_HDR)            count, longest non-empty read, non-empty reads with qualities, skipped reads
//   lengths  L + 1         read length histogram (0 .. L)
//   gc       101           GC% histogram
//   meanq    256           mean-quality histogram, bin = mean + quality_base (a mean lies in
//                          [-quality_base, 255 - quality_base])
//   seq      L x 256       per position, per sequence byte
//   qual     L x 256       per position, per quality byte
//   first    L + 1, 101, 256  per bin of the three histograms: ~(index of the first read that landed in it), 0 =
//                          none (the reference's histograms are dicts in first-seen order, and its median
//                          follows that order; the complement lets a cleared block start at 0 and a
//                          max keep the earliest read, independent of launch order)
constexpr int ST_HDR = 8;
enum { ST_COUNT = 0, ST_LONGEST = 1, ST_WITHQ = 2, ST_SKIPPED = 3 };
constexpr int ST_GC_BINS = 101;
constexpr int ST_MQ_BINS = 256;

ATR_HD long long st_len_off(int L) { (void)L; return ST_HDR; }
ATR_HD long long st_gc_off(int L) { return ST_HDR + (long long)L + 1; }
ATR_HD long long st_mq_off(int L) { return st_gc_off(L) + ST_GC_BINS; }
ATR_HD long long st_seq_off(int L) { return st_mq_off(L) + ST_MQ_BINS; }
ATR_HD long long st_qual_off(int L) { return st_seq_off(L) + (long long)L * 256; }
ATR_HD long long st_first_off(int L) { return st_qual_off(L) + (long long)L * 256; }   // lengths, then gc, then meanq
ATR_HD long long st_words(int L) { return st_first_off(L) + (long long)L + 1 + ST_GC_BINS + ST_MQ_BINS; }

// round(num / den) with Python's round (half to even), den > 0, num of either sign.  Python
// divides the integers into a double first and rounds that; both give the same integer here:
// with den <= 32736 and |num| < 2^24, a quotient that is not a tie lies at least 1 / (2 den)
// >= 1.5e-5 away from the nearest x.5, while the double's rounding error is below
// |num / den| * 2^-53 < 2^-29, so the double never crosses or lands on a tie it is not; an exact
// tie (2 r == den) is representable as a double and rounds to the even neighbour in both.
// Floor division (Python's divmod) keeps r in [0, den) for a negative numerator (mean quality
// below the base), which C's truncating '/' would not.
ATR_HD int st_div_round_even(int num, int den) {
    int q = num / den, r = num - q * den;
    if (r < 0) { q -= 1; r += den; }
    const int twice = 2 * r;
    if (twice > den || (twice == den && (q & 1))) q += 1;
    return q;
}

}  // namespace atr
