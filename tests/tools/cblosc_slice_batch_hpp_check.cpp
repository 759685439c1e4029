// The C++ mirror of the batched C-Blosc-1 slice reads (go-blosc_amd/host/blosc.hpp CBloscGetSliceBatch) against the library: built and run by
// tests/test_cblosc_slice_batch_cpu.py.  A memcpyed frame of a 6 x 10 chunk of 4-byte items needs no decoder, so the selection either comes
// back exact (a device is there) or every accepted job says HB_ERR_NO_DEVICE; what the host refuses is the same either way.
#include <cstdio>
#include <cstring>
#include "../../go-blosc_amd/host/blosc.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    std::vector<int64_t> rc;
    REQUIRE(blosc::CBloscGetSliceBatch({}, {}, rc).empty() && rc.empty());
    blosc::Bytes f(16 + 240);
    const uint8_t head[16] = {2, 1, 0x32, 4, 240, 0, 0, 0, 240, 0, 0, 0, 0, 1, 0, 0};      // memcpyed, nbytes 240, blocksize 240, cbytes 256
    std::memcpy(f.data(), head, 16);
    for (size_t i = 0; i < 240; i++) f[16 + i] = (uint8_t)(i * 3 + 1);
    blosc::Bytes v3 = f;
    v3[0] = 3;
    const std::vector<blosc::SliceJob> jobs = {{0, {6, 10}, {1, 2}, {3, 4}, {2, 2}}, {1, {6, 10}, {0, 0}, {1, 1}, {1, 1}}, {0, {6, 10}, {0, 0}, {3, 1}, {3, 1}},
                                               {0, {6, 10}, {2, 2}, {0, 5}, {1, 1}}, {0, {60}, {7}, {5}, {11}}, {0, {6, 10}, {0, 0}, {2, 2}, {1, 0}}};
    const std::vector<blosc::Bytes> out = blosc::CBloscGetSliceBatch({f, v3}, jobs, rc);
    REQUIRE(out.size() == 6 && rc.size() == 6);
    REQUIRE(rc[1] == HB_ERR_INVALID_VERSION && rc[2] == HB_ERR_BAD_ARG && rc[5] == HB_ERR_BAD_ARG && out[1].empty() && out[2].empty() && out[5].empty());
    if (hb_init() != HB_OK) {
        REQUIRE(rc[0] == HB_ERR_NO_DEVICE && rc[3] == HB_ERR_NO_DEVICE && rc[4] == HB_ERR_NO_DEVICE);
        std::puts("slice mirror ok (no device)");
        return 0;
    }
    REQUIRE(rc[0] == 48 && out[0].size() == 48 && rc[3] == 0 && out[3].empty() && rc[4] == 20 && out[4].size() == 20);
    for (size_t r = 0; r < 3; r++)
        for (size_t c = 0; c < 4; c++)
            for (size_t b = 0; b < 4; b++) REQUIRE(out[0][(r * 4 + c) * 4 + b] == f[16 + ((1 + 2 * r) * 10 + 2 + 2 * c) * 4 + b]);
    for (size_t c = 0; c < 5; c++)
        for (size_t b = 0; b < 4; b++) REQUIRE(out[4][c * 4 + b] == f[16 + (7 + 11 * c) * 4 + b]);
    std::puts("slice mirror ok");
    return 0;
}
