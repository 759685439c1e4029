// The C++ mirror of the batched C-Blosc-1 box writes (go-blosc_amd/host/blosc.hpp CBloscCompressBoxBatch) against the library: built and run by
// tests/test_cblosc_enc_box_batch_cpu.py.  A chunk of 6 x 10 items of 4 bytes is below one matcher chunk, so its frame is memcpyed: 16 header
// bytes and the assembled chunk, which either comes back exact (a device is there) or every accepted job says HB_ERR_NO_DEVICE; what the host
// refuses is the same either way.
#include <cstdio>
#include <cstring>
#include "../../go-blosc_amd/host/blosc.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    std::vector<int64_t> rc;
    REQUIRE(blosc::CBloscCompressBoxBatch({}, rc).empty() && rc.empty());
    // an array of 9 x 13 items, exact size: the box at (4, 5) of shape 5 x 8 is an edge chunk, 4 x 7 of it come from the array
    std::vector<uint8_t> arr(9 * 13 * 4);
    for (size_t i = 0; i < arr.size(); i++) arr[i] = (uint8_t)(i * 5 + 3);
    const uint8_t fill[4] = {0xA1, 0xB2, 0xC3, 0xD4};
    const std::vector<blosc::SrcBox> boxes = {
        {arr.data(), {6, 10}, {6, 10}, {52, 4}},                           // a whole box, strided
        {arr.data() + (4 * 13 + 5) * 4, {6, 10}, {5, 8}, {52, 4}},         // short in both dimensions
        {arr.data(), {6, 10}, {7, 10}, {52, 4}},                           // shape > chunk_shape
        {nullptr, {6, 10}, {0, 10}, {52, 4}},                              // all fill: no source
        {arr.data(), {6, 10}, {6, 10}, {52, 8}},                           // the last stride is not the typesize
        {arr.data(), {1 << 20, 1 << 20}, {1, 1}, {4, 4}},                  // beyond 2 GiB
        {nullptr, {6, 10}, {1, 1}, {52, 4}},                               // a NULL source with an item to read
    };
    const std::vector<blosc::Bytes> out = blosc::CBloscCompressBoxBatch(boxes, rc, fill, 1, 4);
    REQUIRE(out.size() == 7 && rc.size() == 7);
    REQUIRE(rc[2] == HB_ERR_BAD_ARG && rc[4] == HB_ERR_BAD_ARG && rc[5] == HB_ERR_DATA_TOO_LARGE && rc[6] == HB_ERR_BAD_ARG);
    REQUIRE(out[2].empty() && out[4].empty() && out[5].empty() && out[6].empty());
    if (hb_init() != HB_OK) {
        REQUIRE(rc[0] == HB_ERR_NO_DEVICE && rc[1] == HB_ERR_NO_DEVICE && rc[3] == HB_ERR_NO_DEVICE);
        std::puts("enc box mirror ok (no device)");
        return 0;
    }
    for (int k : {0, 1, 3}) REQUIRE(rc[k] == 16 + 240 && out[k].size() == 256 && (out[k][2] & 0x02));
    for (size_t r = 0; r < 6; r++)
        for (size_t c = 0; c < 10; c++)
            for (size_t b = 0; b < 4; b++) {
                const size_t at = 16 + (r * 10 + c) * 4 + b;
                REQUIRE(out[0][at] == arr[(r * 13 + c) * 4 + b]);
                REQUIRE(out[1][at] == (r < 5 && c < 8 ? arr[((4 + r) * 13 + 5 + c) * 4 + b] : fill[b]));
                REQUIRE(out[3][at] == fill[b]);
            }
    std::puts("enc box mirror ok");
    return 0;
}
