// hb_lz4_batch_frame.h — the frame record of the batched matchers (k_match / k_match_fused of hb_lz4_enc.hip take a table of these and a
// chunk -> frame map).  Plain C++, no HIP: hb_lz4_enc.hip fills it for go-blosc frames, hb_cblosc_enc_batch.h for C-Blosc-1 frames.
#pragma once
#include <stdint.h>
#include "../../include/hipblosc.h"

struct EncPlan;                  // hb_lz4_enc.hip (go-blosc frames only)

// ---- batches of frames in ONE set of launches (hb_compress_frames_batch_dev; SURVEY §8 f1 "frame batches") ----
// Chunks are independent and the scan is per frame, so K frames are K segments of one flat chunk space: global chunk g belongs to
// frame chunk_frame[g] and is that frame's chunk g - chunk0; scan tiles never span two frames (tile_frame[t]); descriptors, records
// and tile summaries are indexed globally, positions and stream offsets stay frame-local.  The single-frame launches pass bf = NULL
// and compile to what they were.
struct BatchFrame {
    const uint8_t *src;          // what the matcher reads: the filtered bytes, or the raw input when the filter is fused
    uint8_t *dst;                // frame start
    const uint8_t *memcpy_src;   // what a memcpy frame stores (NULL: the gated batch filter writes the payload)
    hb_result *result;
    EncPlan *plan;
    uint64_t n;
    uint32_t chunk0, nchunks;    // first global chunk / chunks of this frame
    uint32_t tile0, ntiles;      // first global scan tile / tiles of this frame
    uint32_t nblk, pad;          // fused byte shuffle: element blocks of the frame (nchunks = nblk * typesize)
};
static_assert(sizeof(BatchFrame) == 72, "BatchFrame is uploaded as it is");
