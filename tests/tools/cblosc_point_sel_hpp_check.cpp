// The C++ mirror of the prepared C-Blosc-1 point selections (go-blosc_amd/host/blosc.hpp PointSelection, SelJobs) against the library: built
// with -Wall and run by tests/test_cblosc_point_sel_cpu.py.  What the host refuses is the same with and without a device; where a device is
// present a selection is built from host points and asked what it keeps (the device forms of the calls need device memory, which this program
// has none of: they are refused for their arguments here and run in the GPU tests).
#include <cstdio>
#include <cstring>
#include "../../go-blosc_amd/host/blosc.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int code_of(const std::vector<hb_cblosc_sel_job> &jobs, const std::vector<hb_cblosc_point> &pts, int ts) {
    try { blosc::PointSelection::FromPoints(jobs, pts, ts); } catch (const blosc::Error &e) { return e.code(); }
    return HB_OK;
}

int main() {
    // the jobs of a 2 x 3 grid of 4 x 5 chunks: points in three chunks, one coordinate twice (it stays in)
    const std::vector<std::vector<int64_t>> coords = {{0, 7, 3, 0, 7}, {0, 14, 4, 0, 2}};
    std::vector<hb_cblosc_point> pts;
    std::vector<uint32_t> frames;
    const std::vector<hb_cblosc_sel_job> jobs = blosc::SelJobs({2, 3}, {4, 5}, coords, 64, pts, frames);
    REQUIRE(jobs.size() == 3 && frames == std::vector<uint32_t>({0, 3, 5}) && pts.size() == 5);
    REQUIRE(jobs[0].chunk_items == 20 && jobs[0].blocksize == 64 && jobs[0].reserved == 0 && jobs[0].first == 0 && jobs[0].count == 3);
    REQUIRE(jobs[1].first == 3 && jobs[1].count == 1 && jobs[2].first == 4 && jobs[2].count == 1);
    const int64_t want[5][2] = {{0, 0}, {19, 2}, {0, 3}, {17, 4}, {19, 1}};
    for (size_t i = 0; i < 5; i++) REQUIRE(pts[i].item == want[i][0] && pts[i].out == want[i][1]);
    bool threw = false;
    try { blosc::SelJobs({2, 3}, {4, 5}, {{8}, {0}}, 64, pts, frames); } catch (const blosc::Error &e) { threw = e.code() == HB_ERR_BAD_ARG; }
    REQUIRE(threw);
    blosc::SelJobs({2, 3}, {4, 5}, coords, 64, pts, frames);
    // the call as a whole: refused before the device is looked for
    REQUIRE(code_of(jobs, pts, 0) == HB_ERR_BAD_ARG && code_of(jobs, pts, 256) == HB_ERR_BAD_ARG && code_of(jobs, {}, 4) == HB_ERR_BAD_ARG);
    std::vector<hb_cblosc_sel_job> bad = jobs;
    bad[1].reserved = 1;
    REQUIRE(code_of(bad, pts, 4) == HB_ERR_BAD_ARG);
    // an empty object answers like a NULL selection
    blosc::PointSelection none;
    REQUIRE(!none && none.DeviceBytes() == 0 && none.ReadWorkspace({}, {}, {}) == 0 && none.UpdateWorkspace({}, {}) == 0);
    REQUIRE(none.ReadDevice({}, {}, {}, {}, {}, {}, nullptr, 0, nullptr) == HB_ERR_BAD_ARG);
    REQUIRE(none.UpdateDevice({}, {}, {}, {}, {}, {}, nullptr, 0, nullptr) == HB_ERR_BAD_ARG);
    threw = false;
    try { none.Info(0); } catch (const blosc::Error &e) { threw = e.code() == HB_ERR_BAD_ARG; }
    REQUIRE(threw);
    if (hb_init() != HB_OK) {
        REQUIRE(code_of(jobs, pts, 4) == HB_ERR_NO_DEVICE);
        std::puts("point selection mirror ok (no device)");
        return 0;
    }
    blosc::PointSelection sel = blosc::PointSelection::FromPoints(jobs, pts, 4);
    REQUIRE(sel && sel.Jobs() == 3 && sel.TypeSize() == 4 && sel.DeviceBytes() == 5 * 16);
    const hb_cblosc_sel_info a = sel.Info(0), b = sel.Info(2);
    REQUIRE(a.status == HB_OK && a.unique == 0 && a.count == 3 && a.need_items == 4 && a.touched_blocks == 2);      // items 0 and 19: bytes 0 .. 3 and 76 .. 79 in blocks of 64
    REQUIRE(b.status == HB_OK && b.unique == 1 && b.count == 1 && b.need_items == 2 && b.touched_blocks == 1);
    blosc::PointSelection moved = std::move(sel);
    REQUIRE(!sel && moved && moved.Info(1).need_items == 5);
    // a call with arrays of the wrong length is refused here; one with a typesize that is not the selection's by the library
    REQUIRE(moved.ReadDevice({}, {}, {}, {0}, {}, {}, nullptr, 0, nullptr) == HB_ERR_BAD_ARG);
    moved.Close();
    REQUIRE(!moved);
    std::puts("point selection mirror ok");
    return 0;
}
