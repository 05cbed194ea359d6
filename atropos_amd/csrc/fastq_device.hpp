// fastq_device.hpp -- the device helpers that more than one of the FASTQ text kernel files uses
// (fastq_kernels.hip, fastq_emit_kernels.hip, pairtext_kernels.hip).
#ifndef ATR_FASTQ_DEVICE_HPP
#define ATR_FASTQ_DEVICE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace atr {

// the complement table of the pair steps, passed by value in the kernel arguments
struct CompTable256 { uint8_t c[256]; };

// bytes per LDS stage of the staged formatters (emit_staged_kernel, emit_pairs_staged_kernel), an input stage and an
// output image per wave: 2 stages per wave -> 6 waves per CU
constexpr int EMIT_STAGE = 13 * 1024;

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

}  // namespace atr
#endif
