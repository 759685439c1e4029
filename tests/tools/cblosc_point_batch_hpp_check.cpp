// The C++ mirror of the batched C-Blosc-1 point reads (go-blosc_amd/host/blosc.hpp CBloscGetPointBatch) against the library: built and run by
// tests/test_cblosc_point_batch_cpu.py.  A memcpyed frame of 60 items of 4 bytes needs no decoder, so the points either come back exact (a
// device is there) or every accepted job says HB_ERR_NO_DEVICE; what the host refuses is the same either way.
#include <cstdio>
#include <cstring>
#include "../../go-blosc_amd/host/blosc.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    std::vector<int64_t> rc;
    REQUIRE(blosc::CBloscGetPointBatch({}, {}, rc).empty() && rc.empty());
    blosc::Bytes f(16 + 240);
    const uint8_t head[16] = {2, 1, 0x32, 4, 240, 0, 0, 0, 240, 0, 0, 0, 0, 1, 0, 0};      // memcpyed, nbytes 240, blocksize 240, cbytes 256
    std::memcpy(f.data(), head, 16);
    for (size_t i = 0; i < 240; i++) f[16 + i] = (uint8_t)(i * 3 + 1);
    blosc::Bytes v3 = f;
    v3[0] = 3;
    const std::vector<int64_t> items = {59, 0, 0, 31, 7}, outs = {1, 6, 0, 3, 4};
    const std::vector<blosc::PointJob> jobs = {{0, items, outs},                                              // unsorted, a repeat, holes at 2 and 5
                                               {1, {0}, {0}},                                                 // a frame of another version
                                               {0, {0, 60}, {0, 1}},                                          // item 60 of 60
                                               {0, {}, {}},                                                   // no points
                                               {0, {5, -1}, {0, 1}},                                          // negative items are not wrapped
                                               {0, {5, 6}, {0, -1}}};                                         // nor negative positions
    const std::vector<blosc::Bytes> out = blosc::CBloscGetPointBatch({f, v3}, jobs, rc);
    REQUIRE(out.size() == 6 && rc.size() == 6);
    REQUIRE(rc[1] == HB_ERR_INVALID_VERSION && rc[2] == HB_ERR_BAD_ARG && rc[4] == HB_ERR_BAD_ARG && rc[5] == HB_ERR_BAD_ARG && out[1].empty() && out[2].empty() && out[4].empty() &&
            out[5].empty());
    bool threw = false;
    std::vector<int64_t> rc2;
    try { blosc::CBloscGetPointBatch({f}, {{0, {1, 2}, {0}}}, rc2); } catch (const std::exception &) { threw = true; }      // items and outs of different lengths
    REQUIRE(threw);
    if (hb_init() != HB_OK) {
        REQUIRE(rc[0] == HB_ERR_NO_DEVICE && rc[3] == HB_ERR_NO_DEVICE);
        std::puts("point mirror ok (no device)");
        return 0;
    }
    REQUIRE(rc[0] == 20 && out[0].size() == 28 && rc[3] == 0 && out[3].empty());
    for (size_t b = 0; b < 4; b++) REQUIRE(out[0][2 * 4 + b] == 0 && out[0][5 * 4 + b] == 0);
    for (size_t i = 0; i < items.size(); i++)
        for (size_t b = 0; b < 4; b++) REQUIRE(out[0][(size_t)outs[i] * 4 + b] == f[16 + (size_t)items[i] * 4 + b]);
    std::puts("point mirror ok");
    return 0;
}
