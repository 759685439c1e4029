// The C++ mirror of the batched C-Blosc-1 index-list reads (go-blosc_amd/host/blosc.hpp CBloscGetIndexBatch) against the library: built and run
// by tests/test_cblosc_index_batch_cpu.py.  A memcpyed frame of a 6 x 10 chunk of 4-byte items needs no decoder, so the selection either comes
// back exact (a device is there) or every accepted job says HB_ERR_NO_DEVICE; what the host refuses is the same either way.
#include <cstdio>
#include <cstring>
#include "../../go-blosc_amd/host/blosc.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    std::vector<int64_t> rc;
    REQUIRE(blosc::CBloscGetIndexBatch({}, {}, rc).empty() && rc.empty());
    blosc::Bytes f(16 + 240);
    const uint8_t head[16] = {2, 1, 0x32, 4, 240, 0, 0, 0, 240, 0, 0, 0, 0, 1, 0, 0};      // memcpyed, nbytes 240, blocksize 240, cbytes 256
    std::memcpy(f.data(), head, 16);
    for (size_t i = 0; i < 240; i++) f[16 + i] = (uint8_t)(i * 3 + 1);
    blosc::Bytes v3 = f;
    v3[0] = 3;
    const std::vector<int64_t> rows = {5, 0, 0, 3}, cols = {9, 2, 7};
    const std::vector<blosc::IndexJob> jobs = {{0, {6, 10}, {0, 0}, {0, 0}, {1, 1}, {rows, cols}},                // lists on both dimensions
                                               {1, {6, 10}, {0, 0}, {1, 1}, {1, 1}, {{0}, {}}},                   // a frame of another version
                                               {0, {6, 10}, {0, 0}, {0, 1}, {1, 1}, {{0, 6}, {}}},                // index 6 of 6
                                               {0, {6, 10}, {2, 2}, {0, 0}, {1, 1}, {{}, cols}},                  // an empty selection
                                               {0, {6, 10}, {0, 1}, {0, 4}, {1, 2}, {rows, {}}},                  // rows by list, columns 1, 3, 5, 7
                                               {0, {6, 10}, {0, 0}, {0, 2}, {1, 1}, {{-1, 2}, {}}}};              // negative indices are not wrapped
    const std::vector<blosc::Bytes> out = blosc::CBloscGetIndexBatch({f, v3}, jobs, rc);
    REQUIRE(out.size() == 6 && rc.size() == 6);
    REQUIRE(rc[1] == HB_ERR_INVALID_VERSION && rc[2] == HB_ERR_BAD_ARG && rc[5] == HB_ERR_BAD_ARG && out[1].empty() && out[2].empty() && out[5].empty());
    if (hb_init() != HB_OK) {
        REQUIRE(rc[0] == HB_ERR_NO_DEVICE && rc[3] == HB_ERR_NO_DEVICE && rc[4] == HB_ERR_NO_DEVICE);
        std::puts("index mirror ok (no device)");
        return 0;
    }
    REQUIRE(rc[0] == 48 && out[0].size() == 48 && rc[3] == 0 && out[3].empty() && rc[4] == 64 && out[4].size() == 64);
    for (size_t r = 0; r < 4; r++)
        for (size_t c = 0; c < 3; c++)
            for (size_t b = 0; b < 4; b++) REQUIRE(out[0][(r * 3 + c) * 4 + b] == f[16 + ((size_t)rows[r] * 10 + (size_t)cols[c]) * 4 + b]);
    for (size_t r = 0; r < 4; r++)
        for (size_t c = 0; c < 4; c++)
            for (size_t b = 0; b < 4; b++) REQUIRE(out[4][(r * 4 + c) * 4 + b] == f[16 + ((size_t)rows[r] * 10 + 1 + 2 * c) * 4 + b]);
    std::puts("index mirror ok");
    return 0;
}
