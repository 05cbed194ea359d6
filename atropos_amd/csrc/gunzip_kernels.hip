// gunzip_kernels.hip -- BGZF .gz input inflated on the device: the compressed members in HBM -> their text, each at its
// place in the chunk's text tensor.
//
//   atr_bgzf_scan        host: the walk over the member headers (BSIZE, ISIZE) -> where every member starts and where
//                        its text lands (inflate_core.hpp: inf_scan)
//   gunzip_kernel        a workgroup of ONE wave per member.  The member's text (64 KiB), the sorted symbols of the three
//                        codes, the CRC table and the per-lane CRCs live in LDS -- 68.3 KiB, two workgroups per CU.  The
//                        decode and everything it checks: inflate_core.hpp.  A member's only stores to global memory are
//                        its text, after ISIZE and CRC were found right, and its status.
// No inline assembly; every byte written to memory goes out through vector stores or integer atomics.
#include <hip/hip_runtime.h>

#include "atropos_hip.h"
#include "launch_util.hpp"
#include "inflate_core.hpp"

namespace atr {

__global__ __launch_bounds__(INF_NT) void gunzip_kernel(const uint8_t *__restrict__ stream, long long n_stream,
                                                        const long long *__restrict__ member_at, const long long *__restrict__ text_at,
                                                        uint8_t *text, long long capacity, int *status, int *bad) {
    __shared__ InfLds lds;
    const long long m = blockIdx.x;
    inf_crc_table(&lds);
    const long long a0 = member_at[m], a1 = member_at[m + 1], t0 = text_at[m], t1 = text_at[m + 1];
    int st = INF_E_RANGE;
    if (inf_ranges_ok(a0, a1, t0, t1, n_stream, capacity)) {
        InfCtx c;
        c.L = &lds;
        c.src = stream + a0;
        c.msize = (uint32_t)(a1 - a0);
        c.dst = text + t0;
        c.n_out = (uint32_t)(t1 - t0);
        st = inf_member(c);
    }
    if (threadIdx.x == 0) {
        status[m] = st;
        if (st) atomicAdd(bad, 1);
    }
}

}  // namespace atr

using namespace atr;

extern "C" {

int atr_bgzf_scan(const uint8_t *buf, int64_t n_bytes, int64_t max_members, int64_t *member_at, int64_t *text_at,
                  int64_t *n_members, int64_t *covered) {
    if (n_bytes < 0 || max_members < 0 || !member_at || !text_at || !n_members || !covered) return ATR_ERR_INVALID;
    if (n_bytes > 0 && !buf) return ATR_ERR_INVALID;
    return inf_scan(buf, n_bytes, max_members, member_at, text_at, n_members, covered) ? ATR_ERR_INVALID : ATR_OK;
}

int atr_gunzip_members(const uint8_t *d_stream, int64_t n_stream, const int64_t *d_member_at, const int64_t *d_text_at,
                       int64_t n_members, uint8_t *d_text, int64_t text_capacity, int32_t *d_status, int32_t *d_bad, void *stream) {
    if (n_stream < 0 || n_members < 0 || text_capacity < 0) return ATR_ERR_INVALID;
    if (n_stream >= ((int64_t)1 << 32) || text_capacity >= ((int64_t)1 << 32) || n_members > INF_MAX_MEMBERS) return ATR_ERR_UNSUPPORTED;
    if (n_members * 26 > n_stream) return ATR_ERR_INVALID;              // (a member is 26 bytes at the least)
    if (!d_bad) return ATR_ERR_INVALID;
    if (n_members > 0 && (!d_stream || !d_member_at || !d_text_at || !d_text || !d_status)) return ATR_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_bad, 0, 4, s);
    if (e != hipSuccess) return hip_fail(e, "atr_gunzip_members memset");
    if (n_members == 0) return ATR_OK;
    hipLaunchKernelGGL(gunzip_kernel, dim3((unsigned)n_members), dim3(INF_NT), 0, s, d_stream, (long long)n_stream,
                       (const long long *)d_member_at, (const long long *)d_text_at, d_text, (long long)text_capacity, d_status, d_bad);
    e = hipGetLastError();
    return e == hipSuccess ? ATR_OK : hip_fail(e, "atr_gunzip_members launch");
}

}  // extern "C"
