// TEST INFRASTRUCTURE: the CPU twin of the stream gunzip (emu_gunzip_stream.cpp, built from inflate_stream_core.hpp) in a
// program of its own, so that it runs under the address and undefined-behaviour sanitizers
// (tests/test_gunzip_stream_host.py builds and runs it).  Every case gets its stream, its window, its text and its
// workspace in heap blocks of exactly their sizes: a load or a store one byte outside any of them is a report.
//   cases.bin     u32 count, then per case: u32 n_stream, start_bit, window_len, crc_in, capacity, chunk_bytes, the
//                 stream, the window
//   results.bin   per case: i32 status, u32 end_bit, final_seen, crc_out, text_len, the text
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "atropos_hip.h"

extern "C" {
int64_t emu_gunzip_stream_workspace(int64_t n_stream, int64_t chunk_bytes, int64_t text_capacity);
int emu_gunzip_stream(const uint8_t *stream, int64_t n_stream, int64_t start_bit, const uint8_t *window, int32_t window_len,
                      uint32_t crc_in, uint8_t *text, int64_t text_capacity, int64_t chunk_bytes, void *workspace,
                      int64_t workspace_bytes, int64_t *result, void *);
}

static uint32_t u32(FILE *f) {
    uint32_t v = 0;
    if (fread(&v, 4, 1, f) != 1) { fprintf(stderr, "short cases file\n"); exit(2); }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint32_t count = u32(in);
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t n = u32(in), start = u32(in), wlen = u32(in), crc = u32(in), cap = u32(in), cb = u32(in);
        uint8_t *stream = (uint8_t *)malloc(n ? n : 1), *window = (uint8_t *)malloc(wlen ? wlen : 1), *text = (uint8_t *)malloc(cap ? cap : 1);
        if ((n && fread(stream, 1, n, in) != n) || (wlen && fread(window, 1, wlen, in) != wlen)) return 2;
        const int64_t need = emu_gunzip_stream_workspace(n, cb, cap);
        if (need <= 0) return 3;
        void *work = malloc((size_t)need);
        memset(work, 0xa5, (size_t)need);
        int64_t res[8];
        const int rc = emu_gunzip_stream(n ? stream : nullptr, n, start, wlen ? window : nullptr, (int32_t)wlen, crc, cap ? text : nullptr, cap,
                                         cb, work, need, res, nullptr);
        if (rc != 0) return 4;
        const int32_t status = (int32_t)res[0];
        const uint32_t size = status == 0 ? (uint32_t)res[2] : 0u;
        if (size > cap) return 5;
        const uint32_t words[4] = {(uint32_t)res[1], (uint32_t)res[3], (uint32_t)res[4], size};
        fwrite(&status, 4, 1, out);
        fwrite(words, 4, 4, out);
        if (size) fwrite(text, 1, size, out);
        free(stream); free(window); free(text); free(work);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
