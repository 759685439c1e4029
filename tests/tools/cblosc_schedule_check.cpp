// The launch schedule of the C-Blosc-1 stream decoders under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_batch.h -- cb_decode_schedule (the step P and the
// grids of the three decoder launches) and cb_stream_of (the permuted stream order the kernel template k_cb_streams walks).
//   cblosc_schedule_check                 the order visits every index of [0, 8 * mgrp) exactly once, whatever the grid
//   cblosc_schedule_check CASES           one line "nstreams nsplit_all any_small" per case in the file CASES ->
//                                         "nstreams nsplit_all any_small P grid_small grid_lz4 grid_blz" per case on stdout
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// what a kernel of `grid` workgroups decodes: workgroup b takes it = b, b + grid, ... below 8 * mgrp
static int check_order(uint32_t nstreams, uint32_t P, uint32_t grid) {
    const uint32_t mgrp = (nstreams + 7u) / 8u;
    REQUIRE(grid >= 8u && grid % 8u == 0u && grid <= 65536u);
    std::vector<uint8_t> seen((size_t)mgrp * 8u, 0);
    for (uint32_t b = 0; b < grid; b++)
        for (uint32_t it = b; it < mgrp * 8u; it += grid) {
            const uint32_t i = cb_stream_of(it, mgrp, P, grid);
            REQUIRE(i < mgrp * 8u && !seen[i]);
            seen[i] = 1;
        }
    for (uint8_t v : seen) REQUIRE(v == 1);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) {
        FILE *f = std::fopen(argv[1], "r");
        REQUIRE(f != nullptr);
        unsigned nstreams, nsplit, any_small;
        while (std::fscanf(f, "%u %u %u", &nstreams, &nsplit, &any_small) == 3) {
            const CbSchedule S = cb_decode_schedule(nstreams, nsplit, any_small);
            std::printf("%u %u %u %u %u %u %u\n", nstreams, nsplit, any_small, S.P, S.grid_small, S.grid_lz4, S.grid_blz);
        }
        std::fclose(f);
        return 0;
    }
    const uint32_t counts[] = {1u, 7u, 8u, 9u, 63u, 64u, 65u, 1000u, 4099u, 76804u};
    int orders = 0;
    for (uint32_t nstreams : counts)
        for (uint32_t nsplit : {1u, 4u, 16u}) {
            const CbSchedule S = cb_decode_schedule(nstreams, nsplit, 0u);
            const uint32_t mgrp = (nstreams + 7u) / 8u;
            REQUIRE(S.grid_small == (mgrp * 8u < 65536u ? mgrp * 8u : 65536u) && S.grid_blz == S.grid_lz4 && S.grid_lz4 <= S.grid_small);
            REQUIRE(cb_decode_schedule(nstreams, nsplit, 1u).grid_lz4 == S.grid_small);
            for (uint32_t grid : {S.grid_small, 8u, S.grid_lz4}) { if (check_order(nstreams, S.P, grid)) return 1; orders++; }
        }
    // more than one pass per workgroup, and the cap: the cases above have to reach both
    REQUIRE(cb_decode_schedule(76804u, 4u, 0u).grid_lz4 < 65536u && cb_decode_schedule(76804u, 1u, 0u).grid_lz4 == 65536u);
    std::printf("%d orders ok under ASan + UBSan\n", orders);
    return 0;
}
