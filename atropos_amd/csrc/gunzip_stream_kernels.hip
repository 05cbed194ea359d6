// gunzip_stream_kernels.hip -- an ordinary .gz member (no member table) inflated on the device: a slab of its deflate
// data in HBM -> the text of the blocks that end inside it.  The method and everything it checks: inflate_stream_core.hpp.
//
//   ist_find_kernel      a one-wave workgroup per chunk: the chunk's candidate block start
//   ist_decode_kernel    a one-wave workgroup per chunk: symbols with markers into the chunk's room.  LDS: the ring of
//                        33 280 16-bit symbols (65 KiB) and the code tables (3.4 KiB) -- 68.4 KiB, two workgroups per CU
//   ist_chain_kernel     ONE wave: the chain of confirmed chunks, their windows, the decode from known state in between
//   ist_resolve_kernel   a wave per chunk: the markers in front of a confirmed chunk's last 32 KiB
//   ist_crc_kernel       a wave per 16 KiB of final text
//   ist_finish_kernel    one lane: the pieces folded behind crc_in, the result words
// No inline assembly; every byte written to memory goes out through vector stores.
#include <hip/hip_runtime.h>

#include "atropos_hip.h"
#include "launch_util.hpp"
#include "inflate_stream_core.hpp"

namespace atr {

__global__ __launch_bounds__(INF_NT) void ist_find_kernel(IstCall k) {
    __shared__ InfTables lds;
    ist_find(&lds, k, blockIdx.x);
}

__global__ __launch_bounds__(INF_NT) void ist_decode_kernel(IstCall k) {
    __shared__ IstLds lds;
    ist_decode(&lds, k, blockIdx.x);
}

__global__ __launch_bounds__(INF_NT) void ist_chain_kernel(IstCall k) {
    __shared__ IstLds lds;
    ist_chain(&lds, k);
}

__global__ __launch_bounds__(INF_NT) void ist_resolve_kernel(IstCall k) { ist_resolve_chunk(k, blockIdx.x); }

__global__ __launch_bounds__(INF_NT) void ist_crc_kernel(IstCall k) {
    __shared__ InfTables lds;
    inf_crc_table(&lds);
    ist_crc_piece(&lds, k, blockIdx.x);
}

__global__ void ist_finish_kernel(IstCall k, uint32_t crc_in, long long *result) {
    if (threadIdx.x == 0) ist_finish(k, crc_in, (int64_t *)result);
}

}  // namespace atr

using namespace atr;

extern "C" {

int64_t atr_gunzip_stream_workspace(int64_t n_stream, int64_t chunk_bytes, int64_t text_capacity) {
    if (ist_args(n_stream, 0, 0, text_capacity, chunk_bytes)) return ATR_ERR_INVALID;
    return ist_plan(n_stream, chunk_bytes, text_capacity).bytes;
}

int atr_gunzip_stream(const uint8_t *d_stream, int64_t n_stream, int64_t start_bit, const uint8_t *d_window, int32_t window_len,
                      uint32_t crc_in, uint8_t *d_text, int64_t text_capacity, int64_t chunk_bytes, void *d_workspace,
                      int64_t workspace_bytes, int64_t *d_result, void *stream) {
    const int bad = ist_args(n_stream, start_bit, window_len, text_capacity, chunk_bytes);
    if (bad) return bad == -1 ? ATR_ERR_INVALID : ATR_ERR_UNSUPPORTED;
    if (!d_workspace || !d_result || (n_stream > 0 && !d_stream) || (window_len > 0 && !d_window) || (text_capacity > 0 && !d_text))
        return ATR_ERR_INVALID;
    const IstPlan p = ist_plan(n_stream, chunk_bytes, text_capacity);
    if (workspace_bytes < p.bytes) return ATR_ERR_INVALID;
    const IstCall k = ist_call(d_stream, n_stream, start_bit, d_window, window_len, d_text, text_capacity, chunk_bytes, d_workspace);
    hipStream_t s = (hipStream_t)stream;
    const dim3 chunks(k.n_chunks), wave(INF_NT);
    hipLaunchKernelGGL(ist_find_kernel, chunks, wave, 0, s, k);
    hipLaunchKernelGGL(ist_decode_kernel, chunks, wave, 0, s, k);
    hipLaunchKernelGGL(ist_chain_kernel, dim3(1), wave, 0, s, k);
    hipLaunchKernelGGL(ist_resolve_kernel, chunks, wave, 0, s, k);
    hipLaunchKernelGGL(ist_crc_kernel, dim3((unsigned)p.n_pieces), wave, 0, s, k);
    hipLaunchKernelGGL(ist_finish_kernel, dim3(1), dim3(INF_NT), 0, s, k, crc_in, (long long *)d_result);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ATR_OK : hip_fail(e, "atr_gunzip_stream launch");
}

}  // extern "C"
