// The C++ mirror of the batched C-Blosc-1 selection updates (go-blosc_amd/host/blosc.hpp CBloscUpdateIndexBatch) against the library: built and
// run by tests/test_cblosc_upd_index_batch_cpu.py.  A chunk of 6 x 10 items of 4 bytes is below one matcher chunk, so its frames are memcpyed:
// 16 header bytes and the chunk -- the old frame is written here by hand, and the new one either comes back exact (a device is there) or every
// accepted job says HB_ERR_NO_DEVICE; what the host refuses is the same either way.
#include <cstdio>
#include <cstring>
#include "../../go-blosc_amd/host/blosc.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    std::vector<int64_t> rc;
    REQUIRE(blosc::CBloscUpdateIndexBatch({}, rc).empty() && rc.empty());
    // the old chunk, as a memcpyed frame
    std::vector<uint8_t> old(16 + 240);
    const uint8_t head[16] = {2, 1, 0x02 | 0x10 | 0x20, 4, 240, 0, 0, 0, 240, 0, 0, 0, 0, 1, 0, 0};
    memcpy(old.data(), head, 16);
    for (size_t i = 0; i < 240; i++) old[16 + i] = (uint8_t)(i * 7 + 1);
    // the new items: an array of 9 x 13
    std::vector<uint8_t> arr(9 * 13 * 4);
    for (size_t i = 0; i < arr.size(); i++) arr[i] = (uint8_t)(i * 5 + 3);
    const uint8_t fill[4] = {0xA1, 0xB2, 0xC3, 0xD4};
    const void *nothing = (const void *)(uintptr_t)8;                      // an old frame that must not be looked at
    const std::vector<blosc::UpdIndex> jobs = {
        {old.data(), old.size(), arr.data(), {6, 10}, {1, 2}, {3, 3}, {2, 3}, {52, 4}, {}, {}},                       // rows 1, 3, 5 and columns 2, 5, 8 over the old frame
        {nullptr, 0, arr.data(), {6, 10}, {0, 0}, {0, 0}, {1, 1}, {52, 4}, {{4, 0}, {9, 1, 3}}, {{5, 2}, {}}},         // lists, the rows from source rows 5 and 2, over a missing chunk
        {nothing, 999, arr.data(), {6, 10}, {0, 0}, {6, 10}, {1, 1}, {52, 4}, {}, {}},                                // the whole chunk
        {old.data(), old.size(), nullptr, {6, 10}, {3, 3}, {0, 2}, {1, 1}, {52, 4}, {}, {}},                          // an empty count: the old chunk again
        {old.data(), old.size(), arr.data(), {6, 10}, {0, 0}, {0, 0}, {1, 1}, {52, 4}, {{4, 0, 4}, {1}}, {}},          // an index that occurs twice
        {old.data(), old.size(), arr.data(), {6, 10}, {1, 2}, {3, 4}, {2, 3}, {52, 4}, {}, {}},                       // the last column index is 11
        {old.data(), old.size() - 1, arr.data(), {6, 10}, {1, 2}, {3, 3}, {2, 3}, {52, 4}, {}, {}},                   // an old frame cut short
        {nullptr, 0, arr.data(), {1 << 20, 1 << 20}, {0, 0}, {1, 1}, {1, 1}, {4, 4}, {}, {}},                         // beyond 2 GiB
        {nullptr, 0, nullptr, {6, 10}, {1, 1}, {1, 1}, {1, 1}, {52, 4}, {}, {}},                                      // a NULL source with an item to read
    };
    const std::vector<blosc::Bytes> out = blosc::CBloscUpdateIndexBatch(jobs, rc, fill, 1, 4);
    REQUIRE(out.size() == 9 && rc.size() == 9);
    REQUIRE(rc[4] == HB_ERR_BAD_ARG && rc[5] == HB_ERR_BAD_ARG && rc[6] == HB_ERR_INVALID_DATA && rc[7] == HB_ERR_DATA_TOO_LARGE && rc[8] == HB_ERR_BAD_ARG);
    for (int k = 4; k < 9; k++) REQUIRE(out[(size_t)k].empty());
    if (hb_init() != HB_OK) {
        for (int k = 0; k < 4; k++) REQUIRE(rc[(size_t)k] == HB_ERR_NO_DEVICE);
        std::puts("upd index mirror ok (no device)");
        return 0;
    }
    for (int k = 0; k < 4; k++) REQUIRE(rc[(size_t)k] == 16 + 240 && out[(size_t)k].size() == 256 && (out[(size_t)k][2] & 0x02));
    const int lrow[2] = {4, 0}, srow[2] = {5, 2}, lcol[3] = {9, 1, 3};
    for (size_t r = 0; r < 6; r++)
        for (size_t c = 0; c < 10; c++)
            for (size_t b = 0; b < 4; b++) {
                const size_t at = 16 + (r * 10 + c) * 4 + b;
                const bool in0 = r % 2 == 1 && c >= 2 && (c - 2) % 3 == 0;
                REQUIRE(out[0][at] == (in0 ? arr[((r - 1) / 2 * 13 + (c - 2) / 3) * 4 + b] : old[at]));
                int ir = -1, ic = -1;
                for (int i = 0; i < 2; i++) if ((size_t)lrow[i] == r) ir = i;
                for (int i = 0; i < 3; i++) if ((size_t)lcol[i] == c) ic = i;
                REQUIRE(out[1][at] == (ir >= 0 && ic >= 0 ? arr[((size_t)srow[ir] * 13 + (size_t)ic) * 4 + b] : fill[b]));
                REQUIRE(out[2][at] == arr[(r * 13 + c) * 4 + b]);
                REQUIRE(out[3][at] == old[at]);
            }
    std::puts("upd index mirror ok");
    return 0;
}
