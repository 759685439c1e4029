// zlib_dec_check.cpp — the serial zlib decoder of go-blosc_amd/csrc/hb_zlib_dec.h (zl_decode_stream: the CPU statement of what the device
// decoder computes) over a file of records, under ASan + UBSan.  tests/test_cblosc_zlib_cpu.py writes the file from the committed goldens, the directed refusals and
// their mutants and builds this with
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I go-blosc_amd/csrc -o zlib_dec_check tests/tools/zlib_dec_check.cpp
// Record: u32 csize, u32 usize, u32 expect (1: decodes, and crc32 of the bytes follows in `crc`; 0: the library refuses it), u32 crc, then the
// stream.  The stream and the output live in heap blocks of exactly their size, so that any access outside them is a sanitizer report.
// Output: one line per disagreement with the library ("stricter" = refused here, decoded there; "laxer" = the reverse; "other bytes" =
// both decode, to different bytes), and a last line "records R agree A stricter S laxer L other O".  Exit status 0 when the file was read
// through and no record decoded to other bytes than the library's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hb_zlib_dec.h"

static uint32_t crc32_of(const uint8_t *p, size_t n) {
    static uint32_t tab[256];
    if (!tab[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); tab[i] = c; }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: zlib_dec_check RECORDS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    ZlState *S = new ZlState;
    unsigned records = 0, agree = 0, stricter = 0, laxer = 0, other = 0;
    for (;;) {
        uint32_t h[4];
        if (fread(h, 4, 4, f) != 4) break;
        uint8_t *src = (uint8_t *)malloc(h[0] ? h[0] : 1), *dst = (uint8_t *)malloc(h[1] ? h[1] : 1);
        if (fread(src, 1, h[0], f) != h[0]) { fprintf(stderr, "short record %u\n", records); return 2; }
        memset(S, 0xA5, sizeof(ZlState));                                       // (nothing may depend on what an earlier stream left)
        const bool ok = zl_decode_stream(src, h[0], dst, h[1], S);
        const bool same = ok && crc32_of(dst, h[1]) == h[3];
        if (ok && h[2] && same) agree++;
        else if (!ok && !h[2]) agree++;
        else if (!ok && h[2]) { stricter++; printf("record %u: stricter\n", records); }
        else if (ok && !h[2]) { laxer++; printf("record %u: laxer\n", records); }
        else { other++; printf("record %u: other bytes\n", records); }
        records++;
        free(src); free(dst);
    }
    fclose(f);
    delete S;
    printf("records %u agree %u stricter %u laxer %u other %u\n", records, agree, stricter, laxer, other);
    return other ? 1 : 0;
}
