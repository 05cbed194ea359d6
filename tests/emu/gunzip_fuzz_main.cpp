// TEST INFRASTRUCTURE: stand-alone driver of the CPU twin of the device gunzip (emu_gunzip.cpp, inflate_core.hpp with
// -DATR_HOST_EMU), built with -fsanitize=address,undefined by tests/test_gunzip_host.py and run as a subprocess:
// nothing sanitized is loaded into Python.
//
//   gunzip_fuzz <cases> <results>
// <cases>:   u32 count, then per case u32 size and the bytes of one (possibly damaged) member.
// <results>: per case i32 status, u32 text size, and -- status 0 -- the text.
// Every member is run the way the kernel runs it: its range is its bytes, its text range the ISIZE of its last four
// bytes.  The stream and the text are heap blocks of exactly those sizes, so that a load or a store outside them is a
// sanitizer report; a status other than 0 must leave nothing but the member's own text range touched.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" int emu_gunzip_members(const uint8_t *stream, int64_t n_stream, const int64_t *member_at, const int64_t *text_at,
                                  int64_t n_members, uint8_t *text, int64_t text_capacity, int32_t *status, int32_t *bad,
                                  void *);

static uint32_t get32(FILE *f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "gunzip_fuzz: short case file\n"); exit(2); }
    return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

static void put32(FILE *f, uint32_t v) {
    const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    fwrite(b, 1, 4, f);
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: gunzip_fuzz <cases> <results>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "gunzip_fuzz: cannot open the files\n"); return 2; }
    const uint32_t count = get32(in);
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t size = get32(in);
        uint8_t *member = (uint8_t *)malloc(size ? size : 1);
        if (size && fread(member, 1, size, in) != size) { fprintf(stderr, "gunzip_fuzz: short case file\n"); return 2; }
        uint32_t isize = 0;
        if (size >= 4) isize = (uint32_t)member[size - 4] | (uint32_t)member[size - 3] << 8 | (uint32_t)member[size - 2] << 16 |
                               (uint32_t)member[size - 1] << 24;
        const uint32_t room = isize <= 65536 ? isize : 0;   // (a larger ISIZE is refused as a range, before any store)
        uint8_t *text = (uint8_t *)malloc(room ? room : 1);
        memset(text, 0xa5, room ? room : 1);
        const int64_t member_at[2] = {0, (int64_t)size}, text_at[2] = {0, (int64_t)isize};
        int32_t status = -1, bad = -1;
        const int rc = emu_gunzip_members(member, size, member_at, text_at, size >= 26 ? 1 : 0, text, room, &status, &bad, nullptr);
        if (size < 26) status = 1;                          // (fewer bytes than a member has: no member to run)
        else if (rc != 0 || bad != (status != 0)) { fprintf(stderr, "gunzip_fuzz: case %u: rc %d, bad %d, status %d\n", i, rc, bad, status); return 3; }
        put32(out, (uint32_t)status);
        put32(out, status == 0 ? room : 0);
        if (status == 0) fwrite(text, 1, room, out);
        free(text);
        free(member);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
