// The C++ mirror of the batched C-Blosc-1 point updates (go-blosc_amd/host/blosc.hpp CBloscUpdatePointBatch, UpdatePointJobs,
// CBloscUpdateVIndex, CBloscUpdateMask) against the library: built and run by tests/test_cblosc_upd_point_batch_cpu.py.  A chunk of 60 items
// of 4 bytes is below one matcher chunk, so its frames are memcpyed: 16 header bytes and the chunk -- the old frame is written here by hand,
// and the new one either comes back exact (a device is there) or every accepted job says HB_ERR_NO_DEVICE; what the host refuses is the same
// either way.
#include <cstdio>
#include <cstring>
#include "../../go-blosc_amd/host/blosc.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    std::vector<int64_t> rc;
    REQUIRE(blosc::CBloscUpdatePointBatch({}, rc).empty() && rc.empty());
    // the old chunk, as a memcpyed frame
    std::vector<uint8_t> old(16 + 240);
    const uint8_t head[16] = {2, 1, 0x02 | 0x10 | 0x20, 4, 240, 0, 0, 0, 240, 0, 0, 0, 0, 1, 0, 0};
    memcpy(old.data(), head, 16);
    for (size_t i = 0; i < 240; i++) old[16 + i] = (uint8_t)(i * 7 + 1);
    // the new items: 20 of them
    std::vector<uint8_t> arr(20 * 4);
    for (size_t i = 0; i < arr.size(); i++) arr[i] = (uint8_t)(i * 5 + 3);
    const uint8_t fill[4] = {0xA1, 0xB2, 0xC3, 0xD4};
    const std::vector<blosc::UpdPoint> jobs = {
        {old.data(), old.size(), arr.data(), 60, {5, 0, 59}, {0, 1, 19}},                          // three points over the old frame
        {nullptr, 0, arr.data(), 60, {7, 3}, {2, 2}},                                              // one source item for two points, over a missing chunk
        {old.data(), old.size(), nullptr, 60, {}, {}},                                             // no points: the old chunk again
        {nullptr, 0, nullptr, 60, {}, {}},                                                         // ... the all-fill chunk
        {old.data(), old.size(), arr.data(), 60, {4, 0, 4}, {0, 1, 2}},                            // an item that occurs twice
        {old.data(), old.size(), arr.data(), 60, {4, 60}, {0, 1}},                                 // an item outside the chunk
        {old.data(), old.size() - 1, arr.data(), 60, {4}, {0}},                                    // an old frame cut short
        {nullptr, 0, arr.data(), 1ll << 40, {4}, {0}},                                             // beyond 2 GiB
        {nullptr, 0, nullptr, 60, {4}, {0}},                                                       // a NULL source with a point
    };
    const std::vector<blosc::Bytes> out = blosc::CBloscUpdatePointBatch(jobs, rc, fill, 1, 4);
    REQUIRE(out.size() == 9 && rc.size() == 9);
    REQUIRE(rc[4] == HB_ERR_BAD_ARG && rc[5] == HB_ERR_BAD_ARG && rc[6] == HB_ERR_INVALID_DATA && rc[7] == HB_ERR_DATA_TOO_LARGE && rc[8] == HB_ERR_BAD_ARG);
    for (int k = 4; k < 9; k++) REQUIRE(out[(size_t)k].empty());
    // the jobs of a 2-d array of 7 x 9 in chunks of 4 x 5: points in three chunks, one of them twice (the last occurrence counts)
    const std::vector<std::vector<int64_t>> coords = {{0, 6, 3, 0, 6}, {0, 8, 4, 0, 2}};
    const std::vector<blosc::UpdPointChunk> ch = blosc::UpdatePointJobs({7, 9}, {4, 5}, coords);
    REQUIRE(ch.size() == 3 && ch[0].grid == 0 && ch[1].grid == 2 && ch[2].grid == 3);
    REQUIRE(ch[0].job.chunk_items == 20 && ch[0].job.items == std::vector<int64_t>({19, 0}) && ch[0].job.srcs == std::vector<int64_t>({2, 3}));
    REQUIRE(ch[1].job.items == std::vector<int64_t>({12}) && ch[1].job.srcs == std::vector<int64_t>({4}));
    REQUIRE(ch[2].job.items == std::vector<int64_t>({13}) && ch[2].job.srcs == std::vector<int64_t>({1}));
    bool threw = false;
    try { blosc::UpdatePointJobs({7, 9}, {4, 5}, {{7}, {0}}); } catch (const blosc::Error &e) { threw = e.code() == HB_ERR_BAD_ARG; }
    REQUIRE(threw);
    // no point: no frame, no call
    const std::vector<blosc::Bytes> none(4);
    REQUIRE(blosc::CBloscUpdateVIndex(none, {7, 9}, {4, 5}, {{}, {}}, blosc::Bytes(4), 4).empty());
    REQUIRE(blosc::CBloscUpdateMask(none, {7, 9}, {4, 5}, std::vector<uint8_t>(63, 0), blosc::Bytes(4), 4).empty());
    if (hb_init() != HB_OK) {
        for (int k = 0; k < 4; k++) REQUIRE(rc[(size_t)k] == HB_ERR_NO_DEVICE);
        std::puts("upd point mirror ok (no device)");
        return 0;
    }
    for (int k = 0; k < 4; k++) REQUIRE(rc[(size_t)k] == 16 + 240 && out[(size_t)k].size() == 256 && (out[(size_t)k][2] & 0x02));
    for (size_t i = 0; i < 60; i++)
        for (size_t b = 0; b < 4; b++) {
            const size_t at = 16 + i * 4 + b;
            REQUIRE(out[0][at] == (i == 5 ? arr[b] : i == 0 ? arr[4 + b] : i == 59 ? arr[76 + b] : old[at]));
            REQUIRE(out[1][at] == (i == 7 || i == 3 ? arr[8 + b] : fill[b]));
            REQUIRE(out[2][at] == old[at]);
            REQUIRE(out[3][at] == fill[b]);
        }
    // z[mask] = scalar over missing chunks: chunks 0 and 3 get frames, every true entry the scalar, everything else the fill value
    std::vector<uint8_t> mask(63, 0);
    mask[0 * 9 + 1] = mask[6 * 9 + 8] = mask[5 * 9 + 5] = 1;
    const blosc::Bytes scalar = {9, 8, 7, 6};
    const std::map<int64_t, blosc::Bytes> fr = blosc::CBloscUpdateMask(none, {7, 9}, {4, 5}, mask, scalar, 4, 1, fill);
    REQUIRE(fr.size() == 2 && fr.count(0) && fr.count(3));
    for (size_t i = 0; i < 20; i++)
        for (size_t b = 0; b < 4; b++) {
            REQUIRE(fr.at(0)[16 + i * 4 + b] == (i == 1 ? scalar[b] : fill[b]));
            REQUIRE(fr.at(3)[16 + i * 4 + b] == (i == 2 * 5 + 3 || i == 1 * 5 + 0 ? scalar[b] : fill[b]));
        }
    std::puts("upd point mirror ok");
    return 0;
}
