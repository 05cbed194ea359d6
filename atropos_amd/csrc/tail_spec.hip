// tail_spec.hip -- the DP tail of the two-pass pre-pass (tail_filter.hpp) compiled at RUN TIME for one aligner:
// piece_spec.hip includes this file under -DATR_TAIL_SPEC=1, so that the aligner's pre-pass object carries its tail as a
// second kernel; jit.hpp hands it over with a generated tail_spec_config.h (the aligner's parameters as constexpr
// objects, atr::tspec).  Read length, word count and raggedness stay arguments of the kernel.  Never compiled by the
// Makefile (tools/jit/spec_offline.sh builds it on its own with hipcc for inspection of the ISA).
#include "tail_filter.hpp"

// grid: win_blocks window blocks first, the band blocks behind them
#ifndef ATR_TAIL_WAVES
#define ATR_TAIL_WAVES 4
#endif
extern "C" __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ATR_TAIL_WAVES, 8)))
void atr_tail_spec(const uint4 *__restrict__ planes, const int32_t *__restrict__ lens, int nchunks, int max_len,
                   uint4 *__restrict__ out, atr::FastWork wk, int win_blocks) {
    atr::tail_body(planes, lens, nchunks, max_len, out, wk, win_blocks);
}
