// hb_host_stage.h — where the host buffers of a batch lie in their device images (host code only, no HIP call: the staging plans of
// hb_cblosc_*_batch.h, the host forms of hb_batch.hip and the sanitizer programs of tests/tools read it).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

// Inputs.  Host buffers that follow each other EXACTLY (item i + 1 starts where item i ends: slices of one array, a Go shim's staging slab) go up
// in ONE copy instead of one per item (a copy call costs ~7 us: 4096 frames of 100 KB spent 28 ms there): the device image mirrors the span,
// off[i] is the item's distance from the first one.  Nothing but the buffers themselves is read, so adjacency has to be exact; one item alone
// is no span, a NULL item never spans, and `span_align` > 1 asks that every offset in the span be a multiple of it.  Every other item lies
// behind the one before it with `slack` bytes that the kernels' wide loads may touch, at a multiple of `align` (a power of two).
// items[i] indexes p[] and len[].
struct HbUpload {
    bool span;
    size_t bytes;                        // of the device image (a span: of the span itself, nothing behind it)
    std::vector<size_t> off;             // per item
};
static inline HbUpload hb_upload_plan(const std::vector<int> &items, const void *const *p, const size_t *len, size_t slack, size_t align, size_t span_align = 1) {
    HbUpload U{items.size() > 1, 0, std::vector<size_t>(items.size(), 0)};
    size_t at = 0;
    for (size_t i = 0; U.span && i < items.size(); i++) {
        const uint8_t *a = (const uint8_t *)p[items[i]];
        U.span = a && at % span_align == 0 && (i + 1 == items.size() || a + len[items[i]] == (const uint8_t *)p[items[i + 1]]);
        at += len[items[i]];
    }
    for (size_t i = 0; i < items.size(); i++) {
        U.off[i] = U.bytes;
        U.bytes += U.span ? len[items[i]] : (len[items[i]] + slack + align - 1) & ~(align - 1);
    }
    return U;
}

// The plans whose jobs read frames (getitem, boxes, points; PLAN has idx, ioff per frame, span_in, in_bytes): the frames that go up
// (used[k]: a carried job reads frame k) and where, with 64 bytes of slack at 256-byte-aligned offsets.
template <class PLAN>
static inline void hb_upload_plan_frames(PLAN &P, int nframes, const void *const *frame, const size_t *n, const std::vector<uint8_t> &used) {
    for (int k = 0; k < nframes; k++) if (used[(size_t)k]) P.idx.push_back(k);
    const HbUpload U = hb_upload_plan(P.idx, frame, n, 64, 256);
    P.span_in = U.span; P.in_bytes = U.bytes;
    for (size_t i = 0; i < P.idx.size(); i++) P.ioff[(size_t)P.idx[i]] = U.off[i];
}

// Destinations.  Buffers that follow each other inside their own capacities (dst[i + 1] in [dst[i] + nbytes[i], dst[i] + cap[i]]) get a device
// image of the same layout and come down in one copy of `span_bytes`: the bytes between two results lie inside the first one's buffer, which
// the caller handed over for writing (the image is zeroed first).  Every other layout: result i behind result i - 1, with `slack` at a
// multiple of `align`.  items[i] indexes dst[] and cap[]; nbytes[i] is item i's.
struct HbDownload {
    bool span;
    size_t bytes, span_bytes;            // of the device image; of the span (0 without one)
    std::vector<size_t> off;             // per item
};
static inline HbDownload hb_download_plan(const std::vector<int> &items, void *const *dst, const size_t *nbytes, const size_t *cap, size_t slack, size_t align) {
    const size_t m = items.size();
    HbDownload D{m > 1, 0, 0, std::vector<size_t>(m, 0)};
    for (size_t i = 0; D.span && i + 1 < m; i++) {
        const uint8_t *a = (const uint8_t *)dst[items[i]], *b = (const uint8_t *)dst[items[i + 1]];
        D.span = a && b && b >= a + nbytes[i] && b <= a + cap[items[i]];
    }
    for (size_t i = 0; i < m; i++) {
        D.off[i] = D.span ? (size_t)((const uint8_t *)dst[items[i]] - (const uint8_t *)dst[items[0]]) : D.bytes;
        D.bytes += (nbytes[i] + slack + align - 1) & ~(align - 1);
    }
    if (D.span) { D.span_bytes = D.off[m - 1] + nbytes[m - 1]; D.bytes = D.span_bytes + slack; }
    return D;
}
