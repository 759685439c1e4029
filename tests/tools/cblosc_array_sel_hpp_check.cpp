// The C++ mirror of the selections from device masks and coordinate arrays (go-blosc_amd/host/blosc.hpp PointSelection::FromDeviceMask,
// FromDeviceCoords, JobChunks, NPoints) against the library: built with -Wall and run by tests/test_cblosc_array_sel_cpu.py.  What the host
// refuses is the same with and without a device.  This program has no device memory: a call that nothing refuses is made only where it reads
// none -- an empty array, no points -- or where there is no device; the GPU tests run the rest.
#include <cstdio>
#include "../../go-blosc_amd/host/blosc.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Shape = std::vector<int64_t>;
static int mask_code(const Shape &a, const Shape &c, const void *m, int ts) {
    try { blosc::PointSelection::FromDeviceMask(a, c, m, ts, 4096); } catch (const blosc::Error &e) { return e.code(); }
    return HB_OK;
}
static int coords_code(const Shape &a, const Shape &c, const std::vector<const int64_t *> &p, int64_t n, int ts) {
    try { blosc::PointSelection::FromDeviceCoords(a, c, p, n, ts, 4096); } catch (const blosc::Error &e) { return e.code(); }
    return HB_OK;
}

int main() {
    static int64_t mem[8];
    const hb_cblosc_sel_array a = blosc::PointSelection::SelArray({70, 1100}, {32, 513}, 4096);
    REQUIRE(sizeof a == 72 && a.ndim == 2 && a.blocksize == 4096 && a.array_shape[1] == 1100 && a.chunk_shape[0] == 32 && a.array_shape[2] == 0 && a.chunk_shape[3] == 0);
    // refused before the device is looked for
    REQUIRE(mask_code({70, 1100}, {32}, mem, 4) == HB_ERR_BAD_ARG && mask_code({}, {}, mem, 4) == HB_ERR_BAD_ARG && mask_code({1, 1, 1, 1, 1}, {1, 1, 1, 1, 1}, mem, 4) == HB_ERR_BAD_ARG);
    REQUIRE(mask_code({70, 1100}, {32, 0}, mem, 4) == HB_ERR_BAD_ARG && mask_code({70, -1}, {32, 513}, mem, 4) == HB_ERR_BAD_ARG);
    REQUIRE(mask_code({70, 1100}, {32, 513}, mem, 0) == HB_ERR_BAD_ARG && mask_code({70, 1100}, {32, 513}, mem, 256) == HB_ERR_BAD_ARG);
    REQUIRE(mask_code({70, 1100}, {32, 513}, nullptr, 4) == HB_ERR_BAD_ARG);
    REQUIRE(mask_code({1 << 16, 1 << 15}, {512, 512}, mem, 4) == HB_ERR_BAD_ARG);
    REQUIRE(mask_code({70, 1100}, {1 << 20, 1 << 9}, mem, 4) == HB_ERR_DATA_TOO_LARGE);
    REQUIRE(coords_code({70, 1100}, {32, 513}, {mem, mem}, -1, 4) == HB_ERR_BAD_ARG && coords_code({70, 1100}, {32, 513}, {mem}, 1, 4) == HB_ERR_BAD_ARG);
    REQUIRE(coords_code({70, 1100}, {32, 513}, {mem, nullptr}, 1, 4) == HB_ERR_BAD_ARG);
    REQUIRE(coords_code({70, 1100}, {32, 513}, {mem, (const int64_t *)((const char *)mem + 4)}, 1, 4) == HB_ERR_BAD_ARG);
    REQUIRE(coords_code({70, 1100}, {(int64_t)1 << 40, 513}, {mem, mem}, 1, 4) == HB_ERR_DATA_TOO_LARGE);
    // an empty object answers like a NULL selection
    blosc::PointSelection none;
    REQUIRE(!none && none.NPoints() == 0);
    bool threw = false;
    try { none.JobChunks(); } catch (const blosc::Error &e) { threw = e.code() == HB_ERR_BAD_ARG; }
    REQUIRE(threw);
    REQUIRE(hb_cblosc_point_sel_njobs(nullptr) == HB_ERR_BAD_ARG && hb_cblosc_point_sel_npoints(nullptr) == HB_ERR_BAD_ARG);
    REQUIRE(hb_cblosc_point_sel_job_points(nullptr, 0, nullptr, 0) == HB_ERR_BAD_ARG);
    if (hb_init() != HB_OK) {
        REQUIRE(mask_code({70, 1100}, {32, 513}, mem, 4) == HB_ERR_NO_DEVICE && coords_code({70, 1100}, {32, 513}, {mem, mem}, 1, 4) == HB_ERR_NO_DEVICE);
        REQUIRE(mask_code({70, 0}, {32, 513}, nullptr, 4) == HB_ERR_NO_DEVICE && coords_code({70, 1100}, {32, 513}, {}, 0, 4) == HB_ERR_BAD_ARG);
        std::puts("array selection mirror ok (no device)");
        return 0;
    }
    // a device is present: the selections that read no device memory
    blosc::PointSelection e = blosc::PointSelection::FromDeviceMask({70, 0}, {32, 513}, nullptr, 4);
    REQUIRE(e && e.Jobs() == 0 && e.NPoints() == 0 && e.JobChunks().empty() && e.TypeSize() == 4);
    blosc::PointSelection z = blosc::PointSelection::FromDeviceCoords({70, 1100}, {32, 513}, {nullptr, nullptr}, 0, 4);
    REQUIRE(z && z.Jobs() == 0 && z.NPoints() == 0 && z.JobChunks().empty());
    blosc::PointSelection host = blosc::PointSelection::FromPoints({hb_cblosc_sel_job{10, 0, 0, 0, 1}}, {hb_cblosc_point{3, 0}}, 4);
    threw = false;
    try { host.JobChunks(); } catch (const blosc::Error &e2) { threw = e2.code() == HB_ERR_BAD_ARG; }      // not built from an array
    REQUIRE(threw && host.NPoints() == 1);
    std::puts("array selection mirror ok");
    return 0;
}
