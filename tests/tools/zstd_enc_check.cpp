// zstd_enc_check.cpp — the serial zstd writer of go-blosc_amd/csrc/hb_zstd_enc.h (zs_encode_from_lz4: the CPU statement of what k_cbe_zstd
// computes) against the serial decoder of hb_zstd_dec.h, under ASan + UBSan.  tests/test_cblosc_zstd_write_cpu.py writes the cases and builds
// this with
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I go-blosc_amd/csrc -o zstd_enc_check tests/tools/zstd_enc_check.cpp
// Case: u32 n, u32 usize, the LZ4 block (n bytes; n == usize: the plain bytes of a stored stream), the usize bytes it decodes to.
// The block, the expected bytes, the written stream (capacity usize: a stream must be smaller) and the decoded bytes live in heap blocks of
// exactly their size, so that any access outside them is a sanitizer report.  The encoder state is filled with 0xA5 before every case.
// Output file (argv[2]): per case u32 length (0: refused, the stream is stored), then the stream.
// Stdout: one line per failure, and a last line "cases C written W stored S bad B".  Exit status 0 when B == 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hb_zstd_enc.h"

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: zstd_enc_check CASES STREAMS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) { perror(argv[1]); return 2; }
    ZsEncState *E = new ZsEncState;
    ZsState *D = new ZsState;
    unsigned cases = 0, written = 0, stored = 0, bad = 0;
    for (;;) {
        uint32_t h[2];
        if (fread(h, 4, 2, f) != 2) break;
        const uint32_t n = h[0], usize = h[1];
        uint8_t *lz4 = (uint8_t *)malloc(n ? n : 1), *want = (uint8_t *)malloc(usize ? usize : 1);
        uint8_t *out = (uint8_t *)malloc(usize ? usize : 1), *back = (uint8_t *)malloc(usize ? usize : 1);
        if (fread(lz4, 1, n, f) != n || fread(want, 1, usize, f) != usize) { fprintf(stderr, "short case %u\n", cases); return 2; }
        memset(E, 0xA5, sizeof(ZsEncState));                                    // (nothing may depend on what an earlier stream left)
        const uint32_t len = (uint32_t)zs_encode_from_lz4(lz4, n, usize, out, usize, E);
        if (len == 0u) stored++;
        else {
            written++;
            memset(D, 0xA5, sizeof(ZsState));
            if (len >= usize) { bad++; printf("case %u: %u bytes for %u\n", cases, len, usize); }
            else if (!zs_decode_frame(out, len, back, usize, D)) { bad++; printf("case %u: the decoder refuses the stream\n", cases); }
            else if (memcmp(back, want, usize) != 0) { bad++; printf("case %u: other bytes\n", cases); }
        }
        fwrite(&len, 4, 1, g);
        fwrite(out, 1, len, g);
        cases++;
        free(lz4); free(want); free(out); free(back);
    }
    fclose(f); fclose(g);
    delete E; delete D;
    printf("cases %u written %u stored %u bad %u\n", cases, written, stored, bad);
    return bad ? 1 : 0;
}
