// TEST INFRASTRUCTURE: CPU twin of atropos_amd/csrc/gunzip_kernels.hip (atr_bgzf_scan, atr_gunzip_members) built from
// the same per-member source (inflate_core.hpp) with -DATR_HOST_EMU: the uniform decode runs once, everything the
// lanes share is a loop over the kernel's 64 lanes, so that the inflater can be developed, its corner cases checked
// and -- in a stand-alone program (gunzip_fuzz_main.cpp) -- run under sanitizers without a GPU.
#include <stdint.h>
#include <string.h>

#include "emu_abi.hpp"
#include "inflate_core.hpp"

using namespace atr;

extern "C" {

int emu_bgzf_scan(const uint8_t *buf, int64_t n_bytes, int64_t max_members, int64_t *member_at, int64_t *text_at,
                  int64_t *n_members, int64_t *covered) {
    if (n_bytes < 0 || max_members < 0 || !member_at || !text_at || !n_members || !covered) return ATR_ERR_INVALID;
    if (n_bytes > 0 && !buf) return ATR_ERR_INVALID;
    return inf_scan(buf, n_bytes, max_members, member_at, text_at, n_members, covered) ? ATR_ERR_INVALID : ATR_OK;
}
EMU_TWIN(bgzf_scan);

int emu_gunzip_members(const uint8_t *stream, int64_t n_stream, const int64_t *member_at, const int64_t *text_at,
                       int64_t n_members, uint8_t *text, int64_t text_capacity, int32_t *status, int32_t *bad, void *) {
    if (n_stream < 0 || n_members < 0 || text_capacity < 0) return ATR_ERR_INVALID;
    if (n_stream >= ((int64_t)1 << 32) || text_capacity >= ((int64_t)1 << 32) || n_members > INF_MAX_MEMBERS) return ATR_ERR_UNSUPPORTED;
    if (n_members * 26 > n_stream) return ATR_ERR_INVALID;
    if (!bad) return ATR_ERR_INVALID;
    if (n_members > 0 && (!stream || !member_at || !text_at || !text || !status)) return ATR_ERR_INVALID;
    *bad = 0;
    static InfLds lds;                                     // (the emulation is single-threaded)
    inf_crc_table(&lds);
    for (int64_t m = 0; m < n_members; ++m) {
        const int64_t a0 = member_at[m], a1 = member_at[m + 1], t0 = text_at[m], t1 = text_at[m + 1];
        int st = INF_E_RANGE;
        if (inf_ranges_ok(a0, a1, t0, t1, n_stream, text_capacity)) {
            InfCtx c;
            c.L = &lds;
            c.src = stream + a0;
            c.msize = (uint32_t)(a1 - a0);
            c.dst = text + t0;
            c.n_out = (uint32_t)(t1 - t0);
            st = inf_member(c);
        }
        status[m] = st;
        if (st) ++*bad;
    }
    return ATR_OK;
}
EMU_TWIN(gunzip_members);

}  // extern "C"
