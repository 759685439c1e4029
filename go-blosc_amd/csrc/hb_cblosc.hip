// hb_cblosc.hip — SURVEY §8 row f4: frames in the C-Blosc-1 wire format (what go-blosc's README.md:20 claims to read and write and
// blosc.go does not: SURVEY §0.2), decoded on the device.  The format as c-blosc 1.21 writes it (blosc.c blosc_d / blosc_c; checked
// against /opt/conda/lib/libblosc.so.1.21.0, which is also what the tests produce their frames with):
//
//   header  16 bytes { version = 2, versionlz, flags, typesize, nbytes u32, blocksize u32, cbytes u32 }
//           flags: 0x01 byte shuffle, 0x02 memcpyed, 0x04 bit shuffle, 0x10 blocks are not split, bits 5-7 codec format
//           (0 blosclz, 1 lz4 / lz4hc, 2 snappy, 3 zlib, 4 zstd)
//   memcpyed: nbytes raw bytes follow.  Else bstarts: int32[nblocks], the offset of every block from the start of the frame;
//   a block is `typesize` streams (or ONE: flag 0x10, and always the last block when it is shorter than blocksize), a stream
//   is { int32 cbytes, data }: an LZ4 block that decodes to blocksize / nstreams bytes -- or those bytes themselves when
//   cbytes says exactly that size.  The filter works per BLOCK: byte shuffle = the block's elements transposed to `typesize`
//   byte planes (the streams ARE the planes; the bytes behind the last whole element stay where they are); bit shuffle =
//   element bit (byte j, bit k) of all elements of the block gathered in row 8 j + k, eight elements per byte, lowest first --
//   only when the block holds a multiple of 8 elements, else the block is stored unfiltered (shuffle.c blosc_internal_bitshuffle).
//
// Blocks and streams are independent, so there is no discovery problem here: k_cb_plan lists the streams (one lane per block
// walks its cbytes fields), k_cb_streams puts one wavefront on every stream (streams are 8-256 KiB, hundreds to thousands per
// frame), k_cb_unfilter undoes the per-block filter.  LZ4 / LZ4HC and memcpyed frames, and -- once hb_cblosc_accept_codecs(0x3)
// has said so -- BloscLZ (the same decoder behind bz_walk, hb_lz4_region.h), and with bit 4 of that mask zstd: a stream is one Zstandard
// frame, Huffman literals and FSE sequences decoded by one wavefront (hb_zstd_dec.h, cb_decode_zstd_stream), and with 0x100 zlib: a stream is
// one zlib stream, deflate blocks and an Adler-32 (hb_zlib_dec.h, cb_decode_zlib_stream); snappy is not read.
// ONE stream-decode kernel serves every path: k_cb_streams<SPACE, WHICH>, a loop over the permuted stream order with the LZ4, the
// BloscLZ, the small (LDS-resident), the zstd or the zlib decoder as its body.  A SPACE says who owns stream i -- the one frame of the call (CbOneSpace),
// a frame of a batch (CbbSpace), a block record of a getitem / box / slice / update batch (CbgSpace) -- and cb_launch_streams launches
// what the owners need, small, then LZ4, then BloscLZ, then zstd, then zlib, with cb_decode_schedule's grids (hb_cblosc_batch.h), under the profile
// stage names k_cb_decode[_small|_blz|_zstd|_zlib], k_cbb_decode[...] and k_cbg_decode[...] of the three families.
#include "hb_sym_decode.h"
#include "hb_zstd_dec.h"
#include "hb_zstd_enc.h"
#include "hb_zlib_dec.h"

#include <atomic>
#include <cstring>
#include <type_traits>
#include "hb_cblosc_batch.h"       // the flags, cb_nsplit, CbStream / CbPlan, and the host side of the batch
#include "hb_cblosc_enc_batch.h"   // the geometry of a written frame, and the host side of the batched encode
#include "hb_cblosc_getitem_batch.h"   // the geometry of an item range, and the host side of the batched getitem
#include "hb_cblosc_box_batch.h"       // the geometry of a box, the host side of the batched box reads, the gather's index arithmetic
#include "hb_cblosc_slice_batch.h"     // the geometry of a stepped selection, the host side of the batched slice reads, the stepped gather's index arithmetic
#include "hb_cblosc_index_batch.h"     // the geometry of an orthogonal selection, the host side of the batched index-list reads, the index arithmetic of its two gathers
#include "hb_cblosc_point_batch.h"     // the host side of the batched point reads, the point table, the point gather's thread mapping
#include "hb_cblosc_enc_box_batch.h"   // the geometry of a source box, the host side of the batched box writes, the gather's index arithmetic
#include "hb_cblosc_upd_index_batch.h" // the selection updates: refusal, tables, records, and the two scatters' index arithmetic
#include "hb_cblosc_upd_point_batch.h" // the point updates: refusal, point table, records, and the scatter's thread
#include "hb_cblosc_upd_box_batch.h"   // the geometry of an update box, the host side of the batched box updates, the overlay's index arithmetic
#include "hb_cblosc_point_sel.h"       // the prepared point selections: what a selection keeps, its two builders, the builder kernel's thread, the per-call prepares
#include "hb_cblosc_array_sel.h"       // selections from device masks and coordinate arrays: the geometry, the row arithmetic, the bodies of the kernels' threads

// ---- the streams of blocks [b0, b0 + nb) (hb_cblosc_getitem_device: the blocks that cover a range; the others' bstarts entries and streams
// are never read); stream offsets count from the first of these blocks ----
__device__ __forceinline__ void cb_plan_block(const uint8_t *__restrict__ frame, uint32_t nbytes, uint32_t blocksize, uint32_t cbytes, uint32_t typesize, uint32_t flags,
                                              CbPlan *plan, CbStream *streams, uint32_t b0, uint32_t idx, bool own_records = false) {
    const uint32_t nblocks = (nbytes + blocksize - 1) / blocksize;
    const uint32_t b = b0 + idx;
    const uint32_t leftover = nbytes % blocksize;
    const bool lastshort = b + 1 == nblocks && leftover != 0u;
    const uint32_t bsize = lastshort ? leftover : blocksize;
    const uint32_t nsplit_frame = cb_nsplit(flags, typesize, blocksize);
    const uint32_t nsplit = lastshort ? 1u : nsplit_frame;
    const uint32_t neblock = bsize / nsplit;
    CbStream *out = streams + (size_t)idx * nsplit_frame;
    // (own_records: idx == 0 and the records are this block's alone -- k_cbg_plan: the last, shorter block has ONE record, not nsplit_frame)
    const uint32_t nrec = own_records ? nsplit : nsplit_frame;
    for (uint32_t s = 0; s < nrec; s++) { CbStream z; z.src = 0; z.csize = 0; z.dst = 0; z.usize = 0; out[s] = z; }
    uint32_t p = (uint32_t)frame[16 + 4 * b] | ((uint32_t)frame[17 + 4 * b] << 8) | ((uint32_t)frame[18 + 4 * b] << 16) | ((uint32_t)frame[19 + 4 * b] << 24);
    bool bad = neblock == 0u || (uint64_t)neblock * nsplit != bsize;                  // (blosc_c only splits what divides)
    for (uint32_t s = 0; s < nsplit && !bad; s++) {
        if ((uint64_t)p + 4u > cbytes) { bad = true; break; }
        const uint32_t cb = (uint32_t)frame[p] | ((uint32_t)frame[p + 1] << 8) | ((uint32_t)frame[p + 2] << 16) | ((uint32_t)frame[p + 3] << 24);
        p += 4u;
        // (longer than LZ4's worst case: no LZ4 stream of this output.  BloscLZ has no such bound -- literal runs may be as short as one byte, two
        // stream bytes per output byte, and the library decodes that: there the frame's own end is the only limit)
        if (cb == 0u || cb > 0x7FFFFFFFu || (uint64_t)p + cb > cbytes || (cb_is_lz4(flags) && cb > neblock + neblock / 255u + 16u)) { bad = true; break; }
        CbStream st; st.src = p; st.csize = cb; st.dst = idx * blocksize + s * neblock; st.usize = neblock;
        out[s] = st;
        p += cb;
    }
    if (bad) atomicExch(&plan->fail, 1u);
}
__global__ void k_cb_plan(const uint8_t *__restrict__ frame, uint64_t n, uint32_t nbytes, uint32_t blocksize, uint32_t cbytes, uint32_t typesize, uint32_t flags,
                          CbPlan *plan, CbStream *streams, uint32_t b0, uint32_t nb) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nb) return;
    cb_plan_block(frame, nbytes, blocksize, cbytes, typesize, flags, plan, streams, b0, idx);
}

#define CB_SMALL_IN 3072u        // longest stream the small decoder stages (cb_decode_small_stream)
// ---- one wavefront per stream ----
// (the bodies are device functions: the kernel template k_cb_streams below passes the frame, plan and target of whoever owns the stream.
// Everything they are given is wave-uniform, and so is every way out of them.)
__device__ __forceinline__ CbStream cb_load_stream(const CbStream *__restrict__ streams, uint32_t i) {
    CbStream st = streams[i];                                                  // wave-uniform, but it comes out of a vector load: to scalar registers
    st.src = RFL(st.src); st.csize = RFL(st.csize); st.dst = RFL(st.dst); st.usize = RFL(st.usize);
    return st;
}
// The decoder is pass A of the symbolic decoder without the symbols (hb_sym_decode.h): 13 KiB of LDS per wavefront -- an image of the last
// 4 KiB of output, older sources read back from HBM -- so that a dozen streams per CU are in flight.  (First version: the serial
// block decoder with its 64 KiB history in LDS, one wavefront per CU: 21 GB/s on 256 MiB of float32.)
template <int CODEC = RG_LZ4>
__device__ __forceinline__ void cb_decode_stream(const uint8_t *__restrict__ frame, CbPlan *plan, const CbStream st, uint8_t *dst, int small_elsewhere,
                                                 uint8_t *s_win, uint2 *s_tq, uint8_t *s_d, int lane) {
    if (st.usize == 0u) return;
    if (st.csize == st.usize) { wave_copy_g2g(dst + st.dst, frame + st.src, st.usize, lane); return; }      // stored
    if (small_elsewhere && st.usize <= HB_CHUNK && st.csize <= CB_SMALL_IN) return;      // the small decoder has it
    uint32_t out = st.dst;
    bool parked;
    const bool ok = sy_decode_unit<false, RG_PWIN, false, CODEC>(frame + st.src, (uint64_t)st.csize, 0u, st.csize, st.dst, st.dst, out, dst, nullptr, s_win, s_tq, s_d, nullptr,
                                          lane, 1, 0u, 0u, nullptr, nullptr, nullptr, parked, st.dst + st.usize);
    if ((!ok || out != st.dst + st.usize) && lane == 0) atomicExch(&plan->fail, 1u);     // blosc_d: "nbytes != neblock -> -2"
    wave_sync();
}
// Streams of at most one chunk (what hb_cblosc_compress writes: every stream is a 4 KiB chunk of the matcher): stream and output both
// fit into LDS, so the chunk decoder's machinery applies as it is -- window-parallel token parser, one token per lane, copies inside
// the LDS image in dependency rounds (hb_dec_common.h) -- at 17 wavefronts per CU.  The LZ4 decoder leaves these streams alone.
#define CB_SMALL HB_CHUNK
__device__ __forceinline__ void cb_decode_small_stream(const uint8_t *__restrict__ frame, CbPlan *plan, const CbStream st, uint8_t *__restrict__ dst,
                                                       uint8_t *s_in, uint8_t *s_out, uint2 *s_tq, int lane) {
    if (st.usize == 0u || st.usize > CB_SMALL || st.csize == st.usize || st.csize > CB_SMALL_IN) return;      // (stored streams: the LZ4 decoder copies them)
    const uint8_t *g = frame + st.src;
    const uint32_t sh = (uint32_t)((uintptr_t)g & 15u), slen = st.csize;           // slen < usize <= 4096
    wave_sync();
    {
        const u32x4 *ga = (const u32x4 *)(g - sh);
        const uint32_t nv = (sh + slen + 15u) >> 4;
        for (uint32_t k = lane; k < nv; k += 64) ((u32x4 *)s_in)[k] = ga[k];
    }
    wave_sync();
    uint32_t si = 0, di = 0, nq = 0;
    bool ok = true, done = false;
    while (ok && !done) {
        const bool stop = dec_fill(s_in, sh, slen, slen, si, nq, s_tq, lane);
        bool rewound = false;
        if (!dec_drain(s_in, (int)sh, s_out, st.usize, 0u, di, si, nq, s_tq, stop, rewound, lane) || rewound) { ok = false; break; }      // (64 at a time; all of them when the parser stopped)
        if (si == slen) { done = true; break; }
        if (!stop) continue;
        // one sequence the slow way: a length extension of several bytes, or the end of the stream
        const uint32_t tok = RFL((uint32_t)s_in[sh + si]);
        si++;
        uint32_t ll = tok >> 4;
        if (ll == 15u && !dec_read_ext(s_in, (int)sh, 0u, slen, g, slen, si, ll, lane)) { ok = false; break; }
        if (ll > slen - si || ll > st.usize - di) { ok = false; break; }
        for (uint32_t k = lane; k < ll; k += 64) s_out[di + k] = s_in[sh + si + k];
        si += ll; di += ll;
        if (si == slen) { if (tok & 15u) ok = false; done = true; break; }            // the final, literal-only sequence
        if (slen - si < 2u) { ok = false; break; }
        const uint32_t off = RFL((uint32_t)s_in[sh + si] | ((uint32_t)s_in[sh + si + 1u] << 8));
        si += 2u;
        uint32_t ml = (tok & 15u) + 4u;
        if ((tok & 15u) == 15u && !dec_read_ext(s_in, (int)sh, 0u, slen, g, slen, si, ml, lane)) { ok = false; break; }
        if (off == 0u || off > di || ml > st.usize - di) { ok = false; break; }
        wave_sync();
        dec_match_copy(s_out, di, off, ml, lane);
        di += ml;
        wave_sync();
    }
    if (!ok || di != st.usize) { if (lane == 0) atomicExch(&plan->fail, 1u); return; }
    wave_sync();
    uint8_t *o = dst + st.dst;
    for (uint32_t k = (uint32_t)lane * 16u; k + 16u <= st.usize; k += 1024u) st16u(o + k, *(const u32x4 *)(s_out + k));
    const uint32_t t0 = st.usize & ~15u;
    if (t0 + (uint32_t)lane < st.usize) o[t0 + lane] = s_out[t0 + lane];
}
// ---- zstd streams (codec format 4; accepted once hb_cblosc_accept_codecs has set bit 4): one wavefront per stream, zstd block by zstd block.
// The format logic is hb_zstd_dec.h, the same functions the host runs serially: one lane parses the headers and builds the FSE tables in LDS
// (ZsState), the wave fills the Huffman table, four lanes (one for a single stream) decode the Huffman streams, one lane decodes up to 64
// sequences into a queue and has checked every length and offset by then, and the wave executes the queue: literal runs and matches are
// wave-wide copies straight in global memory.  Huffman literals wait in the tail of the stream's own output (the no-overlap argument is at the
// top of hb_zstd_dec.h), so the decoder needs no workspace of its own.  A match may copy bytes this wave stored a moment ago: it reads them
// only behind sy_sync() (hb_sym_decode.h: every store of the wave has reached the cache the CU reads through, later loads are not started
// early) -- once per match whose source reaches above `synced`, the output position at the last such wait, not once per sequence. ----
__device__ __forceinline__ void zs_wave_fill(uint8_t *d, uint32_t v, uint32_t n, int lane) {
    uint32_t head = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u);
    if (head > n) head = n;
    if ((uint32_t)lane < head) d[lane] = (uint8_t)v;
    const uint32_t body = (n - head) >> 2, w = v * 0x01010101u;
    for (uint32_t i = lane; i < body; i += 64) *(uint32_t *)(d + head + 4u * i) = w;
    const uint32_t done = head + 4u * body;
    if (done + (uint32_t)lane < n) d[done + lane] = (uint8_t)v;
}
// `len` literals of the block at hand to out + o; `used`: how many went out before
__device__ __forceinline__ void zs_wave_literals(const uint8_t *src, uint8_t *out, uint32_t lt, uint32_t lat, uint32_t used, uint32_t o, uint32_t len, int lane) {
    if (len == 0u) return;
    if (lt == ZS_LIT_RLE) zs_wave_fill(out + o, src[lat], len, lane);
    else wave_copy_g2g(out + o, (lt == ZS_LIT_RAW ? src : (const uint8_t *)out) + lat + used, len, lane);      // (the tail: o <= lat + used, a copy downwards, chunk by chunk)
}
// An overlapping match (off < ml) repeats the `off` bytes in front of it: byte k is byte k % off of them.  The first 256 bytes go out four
// per lane as one word (one modulo per lane, then a wrap-around count); the rest is copied from what the match has written itself, a whole
// number of periods back, so that every pass is a copy without overlap, at least doubles what is there, and moves 16 bytes per lane -- a
// run of 128 KiB (off 1) is ten passes.  The caller has waited for the bytes in front of o; every pass waits for the pass before it.
__device__ __forceinline__ void zs_wave_overlap(uint8_t *out, uint32_t o, uint32_t off, uint32_t ml, int lane) {
    const uint32_t from = o - off, n1 = ml < 256u ? ml : 256u, k = 4u * (uint32_t)lane;
    if (k < n1) {
        const uint32_t m = n1 - k < 4u ? n1 - k : 4u;
        uint32_t i = k % off, v = 0u;
        for (uint32_t j = 0; j < m; j++) { v |= (uint32_t)out[from + i] << (8u * j); i = i + 1u == off ? 0u : i + 1u; }
        if (m == 4u) st4u(out + o + k, v);
        else for (uint32_t j = 0; j < m; j++) out[o + k + j] = (uint8_t)(v >> (8u * j));
    }
    for (uint32_t done = n1; done < ml; ) {                                     // (every pass at least doubles `done`: log2(ml / 256) + 1 passes)
        sy_sync();
        const uint32_t back = (off + done) / off * off;                         // a multiple of the period, done < back <= off + done: the source starts at or behind o - off
        const uint32_t len = ml - done < back ? ml - done : back;
        wave_copy_g2g(out + o + done, out + o + done - back, len, lane);
        done += len;
    }
}
// one compressed block; S->ip at its content, S->produced = o.  false: refused.
__device__ __forceinline__ bool zs_wave_block(ZsState *S, const uint8_t *src, uint8_t *out, const uint32_t U, const uint32_t block_end, uint32_t &o, uint32_t &synced, int lane) {
    const uint32_t block_out = o;
    if (lane == 0) S->ok = zs_literals_header(S, src, U) ? 1u : 0u;
    wave_sync();
    if (!RFL(S->ok)) return false;
    const uint32_t lt = RFL(S->lit_type), lsize = RFL(S->lit_size), lat = RFL(S->lit_at), ns = RFL(S->nstreams);
    if (RFL(S->lit_new_tree)) { zs_huf_fill(S, (uint32_t)lane, 64u); wave_sync(); }
    if (ns) {
        bool good = true;
        if ((uint32_t)lane < ns)
            good = zs_huf_stream(S->huf, S->huf_log, src + S->hs_at[lane], S->hs_n[lane], out + lat + S->hs_cnt[0] * (uint32_t)lane, S->hs_cnt[lane]);
        if (hb_ballot(!good)) return false;
        sy_sync();                                                              // the literals are read back below
    }
    if (lane == 0) S->ok = zs_sequences_header(S, src, block_end) ? 1u : 0u;
    wave_sync();
    if (!RFL(S->ok)) return false;
    const uint32_t nseq = RFL(S->nseq);
    uint32_t used = 0u;
    for (uint32_t done = 0u; done < nseq; done += ZS_QUEUE) {                   // (nseq / 64 passes)
        if (lane == 0) { bool k; S->produced = o; zs_seq_batch(S, src, U, &k); S->ok = k ? 1u : 0u; }
        wave_sync();
        if (!RFL(S->ok)) return false;
        const uint32_t cnt = nseq - done < ZS_QUEUE ? nseq - done : ZS_QUEUE;
        for (uint32_t q = 0; q < cnt; q++) {
            const uint32_t ll = RFL(S->q_ll[q]), ml = RFL(S->q_ml[q]), off = RFL(S->q_off[q]);
            zs_wave_literals(src, out, lt, lat, used, o, ll, lane);
            used += ll; o += ll;
            const uint32_t from = o - off;
            if (from + (ml < off ? ml : off) > synced) { sy_sync(); synced = o; }      // the source holds bytes stored since the last wait
            if (off >= ml) wave_copy_g2g(out + o, out + from, ml, lane);
            else zs_wave_overlap(out, o, off, ml, lane);
            o += ml;
        }
        wave_sync();
    }
    const uint32_t tail = lsize - used;                                         // the literals behind the last sequence
    if (tail > U - o) return false;
    zs_wave_literals(src, out, lt, lat, used, o, tail, lane);
    o += tail;
    if (lt == ZS_LIT_HUF) { sy_sync(); synced = o; }                            // (the next block's tail may be written over bytes this copy read)
    return o - block_out <= ZS_BLOCK_MAX;
}
__device__ __forceinline__ void cb_decode_zstd_stream(const uint8_t *__restrict__ frame, CbPlan *plan, const CbStream st, uint8_t *dst, ZsState *S, int lane) {
    if (st.usize == 0u) return;
    if (st.csize == st.usize) { wave_copy_g2g(dst + st.dst, frame + st.src, st.usize, lane); return; }      // stored
    const uint8_t *src = frame + st.src;
    uint8_t *out = dst + st.dst;
    const uint32_t N = st.csize, U = st.usize;
    wave_sync();
    if (lane == 0) S->ok = (N <= 0x7FFFFFFFu && zs_frame_header(S, src, N, U)) ? 1u : 0u;
    wave_sync();
    bool ok = RFL(S->ok) != 0u, last = false;
    uint32_t o = 0u, synced = 0u;
    for (uint32_t nb = 0u; ok && !last && nb <= N / 3u; nb++) {                 // (a block takes 3 bytes at least)
        if (lane == 0) { S->produced = o; S->ok = zs_block_header(S, src, N, U) ? 1u : 0u; }
        wave_sync();
        if (!RFL(S->ok)) { ok = false; break; }
        const uint32_t type = RFL(S->b_type), size = RFL(S->b_size), ip = RFL(S->ip);
        last = RFL(S->b_last) != 0u;
        wave_sync();
        if (type == 0u) { wave_copy_g2g(out + o, src + ip, size, lane); o += size; if (lane == 0) S->ip = ip + size; }
        else if (type == 1u) { zs_wave_fill(out + o, src[ip], size, lane); o += size; if (lane == 0) S->ip = ip + 1u; }
        else ok = zs_wave_block(S, src, out, U, ip + size, o, synced, lane);
        wave_sync();
    }
    if (ok) {
        if (lane == 0) { S->produced = o; S->ok = (last && zs_frame_end(S, N, U)) ? 1u : 0u; }
        wave_sync();
        ok = RFL(S->ok) != 0u;
    }
    if (!ok && lane == 0) atomicExch(&plan->fail, 1u);
    wave_sync();
}
// ---- zlib streams (codec format 3; accepted once hb_cblosc_accept_codecs has set 0x100): one wavefront per stream, deflate block by deflate
// block.  The format logic is hb_zlib_dec.h, the same functions the host runs serially: one lane parses the block header, reads a dynamic
// block's code lengths and puts both codes into canonical form (ZlState in LDS), the wave fills the two root tables, one lane decodes symbols
// into a queue of up to 64 {literal run, match} entries -- the literal bytes into an LDS buffer, every length and distance checked by then --
// and the wave executes the queue: literal runs are wave-wide copies out of LDS, matches the copies of the zstd body above (zs_wave_overlap
// for the overlapping ones), stored blocks a wave-wide copy.  Literals are inline in deflate: no workspace, nothing parked in the output.
// A match reads bytes this wave stored a moment ago only behind sy_sync(), by the `synced` watermark rule of the zstd body.  The Adler-32 is
// the whole wave's: zl_wave_adler reads the finished output back. ----
// literals out of LDS: single bytes up to the destination's next word, words put together from four LDS bytes, single bytes behind them
__device__ __forceinline__ void zl_wave_lits(uint8_t *d, const uint8_t *lit, uint32_t n, int lane) {
    uint32_t head = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u);
    if (head > n) head = n;
    if ((uint32_t)lane < head) d[lane] = lit[lane];
    const uint32_t body = (n - head) >> 2;
    for (uint32_t i = lane; i < body; i += 64) {
        const uint8_t *p = lit + head + 4u * i;
        *(uint32_t *)(d + head + 4u * i) = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    const uint32_t done = head + 4u * body;
    if (done + (uint32_t)lane < n) d[done + lane] = lit[done + lane];
}
// Adler-32 of out[0, U) by the wave; the caller has waited for the stores (sy_sync).  The output goes by in chunks of C <= 16384 bytes, a
// chunk in tiles of 1024: lane l takes the 16 bytes at 1024 t + 16 l of tile t.  With (s1, s2) in front of a chunk of C bytes b_i,
//     s1' = s1 + sum b_i,      s2' = s2 + C s1 + sum (C - i) b_i,
// and for i = 1024 t + 16 l + j:  C - i = (C - 1024 t - 16 l - 16) + (16 - j), so a lane adds per tile  A = sum_j b_j  to a  and
// (C - 1024 t - 16 l - 16) A + sum_j (16 - j) b_j  to x  (bytes behind the chunk's end count as zeros; the first factor may then be "negative",
// the lane's true total is not, and unsigned arithmetic gives it).  The chunk bound: A <= 16 * 255 = 4080, sum_j (16 - j) b_j <= 136 * 255 =
// 34680, so after the C / 1024 = 16 tiles of a chunk  x <= 16 * (16384 * 4080 + 34680) = 1 070 102 400 < 2^32  and  a <= 65280 -- the serial
// form's 5552 bytes are passed because a lane sees a 64th of the bytes, and 32 tiles (4 279 299 840) would still fit, with 0.4 % to spare:
// 16 it is.  Then x is reduced modulo 65521 in every lane, the 64 values (< 2^22 together) and the 64 a (< 2^22) are added up across the
// wave, and s2' = (s2 + (C mod 65521) s1 + sum x) mod 65521 with s1, s2 < 65521 and C <= 16384: below 2^31.
__device__ __forceinline__ uint32_t zl_wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t zl_wave_adler(const uint8_t *out, uint32_t U, int lane) {
    uint32_t s1 = 1u, s2 = 0u;
    for (uint32_t c0 = 0; c0 < U; c0 += 16384u) {                               // (U / 16384 passes)
        const uint32_t C = U - c0 < 16384u ? U - c0 : 16384u;
        uint32_t a = 0u, x = 0u;
        for (uint32_t t0 = 0; t0 < C; t0 += 1024u) {
            const uint32_t i = t0 + 16u * (uint32_t)lane;
            uint32_t A = 0u, W = 0u;
            if (i + 16u <= C) {
                const u32x4 v = ld16u(out + c0 + i);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    const uint32_t b0 = w[k] & 255u, b1 = (w[k] >> 8) & 255u, b2 = (w[k] >> 16) & 255u, b3 = w[k] >> 24;
                    A += b0 + b1 + b2 + b3;
                    W += (16u - 4u * k) * b0 + (15u - 4u * k) * b1 + (14u - 4u * k) * b2 + (13u - 4u * k) * b3;
                }
            } else if (i < C) {
                for (uint32_t j = 0; i + j < C; j++) { const uint32_t b = out[c0 + i + j]; A += b; W += (16u - j) * b; }      // (the chunk's last lane: under 16 bytes)
            }
            a += A; x += (C - i - 16u) * A + W;
        }
        x %= ZL_ADLER;
        a = zl_wave_sum(a); x = zl_wave_sum(x);
        s2 = (s2 + (C % ZL_ADLER) * s1 + x) % ZL_ADLER;
        s1 = (s1 + a) % ZL_ADLER;
    }
    return (s2 << 16) | s1;
}
__device__ __forceinline__ void cb_decode_zlib_stream(const uint8_t *__restrict__ frame, CbPlan *plan, const CbStream st, uint8_t *dst, ZlState *S, int lane) {
    if (st.usize == 0u) return;
    if (st.csize == st.usize) { wave_copy_g2g(dst + st.dst, frame + st.src, st.usize, lane); return; }      // stored
    const uint8_t *src = frame + st.src;
    uint8_t *out = dst + st.dst;
    const uint32_t N = st.csize, U = st.usize;
    wave_sync();
    if (lane == 0) S->ok = zl_header(S, src, N) ? 1u : 0u;
    wave_sync();
    bool ok = RFL(S->ok) != 0u, last = false;
    uint32_t o = 0u, synced = 0u;
    for (uint32_t nb = 0u; ok && !last && nb <= 8u * N / 3u; nb++) {            // (a block takes 3 bits at least; N < 2^28 behind zl_header)
        if (lane == 0) { S->produced = o; S->ok = zl_block_header(S, src, N) ? 1u : 0u; }
        wave_sync();
        if (!RFL(S->ok)) { ok = false; break; }
        last = RFL(S->b_final) != 0u;
        if (RFL(S->b_type) == 0u) {
            const uint32_t len = RFL(S->b_len);
            if (len > U - o) { ok = false; break; }
            wave_copy_g2g(out + o, src + RFL(S->b_at), len, lane);
            o += len;
            wave_sync();
            continue;
        }
        zl_root_clear(S->lfast, ZL_LROOT, (uint32_t)lane, 64u); zl_root_clear(S->dfast, ZL_DROOT, (uint32_t)lane, 64u);
        wave_sync();
        zl_root_fill(S->lfast, ZL_LROOT, S->lcode, S->lsym, S->lens, S->nlen, (uint32_t)lane, 64u);
        zl_root_fill(S->dfast, ZL_DROOT, S->dcode, S->dsym, S->lens + S->nlen, S->ndist, (uint32_t)lane, 64u);
        wave_sync();
        for (bool eob = false; !eob; ) {                                        // (every pass but the last takes ZL_QUEUE entries or ZL_LITBUF bytes off the stream)
            if (lane == 0) { S->produced = o; S->ok = zl_symbols(S, src, N, U) ? 1u : 0u; }
            wave_sync();
            if (!RFL(S->ok)) { ok = false; break; }
            const uint32_t cnt = RFL(S->nq);
            eob = RFL(S->eob) != 0u;
            uint32_t lat = 0u;
            for (uint32_t q = 0; q < cnt; q++) {
                const uint32_t ll = RFL(S->q_ll[q]), ml = RFL(S->q_ml[q]), off = RFL(S->q_dist[q]);
                if (ll) zl_wave_lits(out + o, S->lit + lat, ll, lane);
                o += ll; lat += ll;
                if (ml == 0u) continue;
                const uint32_t from = o - off;
                if (from + (ml < off ? ml : off) > synced) { sy_sync(); synced = o; }      // the source holds bytes stored since the last wait
                if (off >= ml) wave_copy_g2g(out + o, out + from, ml, lane);
                else zs_wave_overlap(out, o, off, ml, lane);
                o += ml;
            }
            wave_sync();
        }
    }
    if (ok && last) {
        sy_sync();                                                              // the output is read back
#ifdef CB_ZLIB_LAB_NO_ADLER                                                      // a measurement build (tools/cblosc_zlib_rates.py --no-adler-into): the trailer on trust
#warning "CB_ZLIB_LAB_NO_ADLER: this library does not verify zlib checksums; it exports hb_cblosc_lab_no_adler and is for tools/cblosc_zlib_rates.py alone"
        const uint32_t adler = zl_trailer(S, src, N);
#else
        const uint32_t adler = zl_wave_adler(out, o, lane);
#endif
        if (lane == 0) { S->produced = o; S->ok = zl_stream_end(S, src, N, U, adler) ? 1u : 0u; }
        wave_sync();
        ok = RFL(S->ok) != 0u;
    } else ok = false;
    if (!ok && lane == 0) atomicExch(&plan->fail, 1u);
    wave_sync();
}
// ---- who owns stream i: a space gives the unified loop below the wave-uniform context of a stream -- the compressed frame, the plan to read
// and to fail, where the decoded bytes go, the owner's codec format (each decoder passes the other codecs' owners by), whether its streams are at most one chunk ("small": an LZ4
// owner only).  The owner index and the fail word come out of vector loads and go through RFL: the bodies above contain wave_sync. ----
struct CbCtx { const uint8_t *frame; CbPlan *plan; uint8_t *target; uint32_t codec; bool small; };
// What the batches' spaces look up -- frame and block records, stream prefixes -- went up before the launch and nobody writes it while a kernel
// runs.  It is read through the constant address space, so that these wave-uniform reads are scalar loads: a `const T *__restrict__` kernel
// argument gets that by itself, a pointer inside an argument struct carries no such promise (as vector loads they cost k_cbb_decode 6 %:
// profiles/cblosc_decode_unify_ab.json, first_build_ms).
#define CB_RO(T) const __attribute__((address_space(4))) T
template <class T>
__device__ __forceinline__ CB_RO(T) *cb_ro(const T *p) { return (CB_RO(T) *)(uintptr_t)p; }
// one frame (hb_cblosc_decompress_dev, hb_cblosc_getitem_device): what the host decided, for every stream
struct CbOneSpace {
    const uint8_t *frame; CbPlan *plan; uint8_t *target; int codec, small;
    static constexpr bool one_plan = true;                                 // one owner: the kernel tests its fail word once, on entry (per stream: +2.7 % on k_cb_decode, second_build_ms of the same file)
    __device__ __forceinline__ CbCtx operator()(uint32_t) const { return CbCtx{frame, plan, target, (uint32_t)codec, small != 0}; }
};
// a batch of whole frames: the frame that owns the stream -- its staged copy, or its destination when there is no filter to undo
struct CbbSpace {
    const CbbFrame *frames; CbPlan *plans; const uint32_t *str0; uint32_t nframes; uint8_t *work;
    static constexpr bool one_plan = false;
    __device__ __forceinline__ CbCtx operator()(uint32_t i) const {
        const uint32_t k = RFL(hb_owner(cb_ro(str0), nframes, i));
        CB_RO(CbbFrame) &F = cb_ro(frames)[k];
        return CbCtx{F.frame, plans + k, F.stage_off ? work + F.stage_off : F.dst, F.flags >> 5, F.small != 0u};
    }
};
// a batch of block records (the getitem, box, slice and update batches): the record's own plan, its staged copy as the target (also without a
// filter: a stream cannot be decoded in part)
struct CbgSpace {
    const CbgFrame *frames; const CbgBlock *blocks; CbPlan *plans; const uint32_t *str0; uint32_t nblk; uint8_t *work;
    static constexpr bool one_plan = false;
    __device__ __forceinline__ CbCtx operator()(uint32_t i) const {
        const uint32_t x = RFL(hb_owner(cb_ro(str0), nblk, i));
        CB_RO(CbgBlock) &K = cb_ro(blocks)[x];
        CB_RO(CbgFrame) &F = cb_ro(frames)[K.frame];
        return CbCtx{F.frame, plans + x, work + K.stage_off, F.flags >> 5, F.small != 0u};
    }
};
// The one stream-decode kernel: one wavefront per stream of the space, in the permuted order (cb_stream_of) over all of it; the host's grids
// are cb_decode_schedule's.  WHICH is the decoder: LZ4 (stored streams of LZ4 owners are copied here; with the small decoder launched, the
// short streams of small owners are left to it), BloscLZ (the same decoder behind bz_walk, hb_lz4_region.h, stored streams included: an owner
// has one codec, so each passes the others' owners by), the small decoder (small owners only: it selects by that and by size), or zstd
// (cb_decode_zstd_stream above, stored streams of zstd owners included), or zlib (cb_decode_zlib_stream, likewise).
// In a batch a stream is skipped once its owner's plan has failed -- one value for the whole wave: nobody is left behind at a wave_sync.
enum { CBW_LZ4 = 0, CBW_BLZ, CBW_SMALL, CBW_ZSTD, CBW_ZLIB };
template <class SPACE, int WHICH>
__global__ __launch_bounds__(64) void k_cb_streams(SPACE sp, const CbStream *__restrict__ streams, uint32_t nstreams, int small_launched, uint32_t P) {
    __shared__ __attribute__((aligned(16))) uint2 s_tq[DTQ];
    const int lane = threadIdx.x;
    const uint32_t mgrp = (nstreams + 7u) / 8u;
    if constexpr (SPACE::one_plan) { if (sp(0u).plan->fail) return; }
    for (uint32_t it = blockIdx.x; it < mgrp * 8u; it += gridDim.x) {
        const uint32_t i = cb_stream_of(it, mgrp, P, gridDim.x);
        if (i >= nstreams) continue;
        const CbCtx c = sp(i);
        if constexpr (!SPACE::one_plan) { if (RFL(c.plan->fail)) continue; }
        if constexpr (WHICH == CBW_SMALL) {
            __shared__ __attribute__((aligned(16))) uint8_t s_in[CB_SMALL_IN + 64 + 128];
            __shared__ __attribute__((aligned(16))) uint8_t s_out[CB_SMALL + 64];
            if (!c.small) continue;
            cb_decode_small_stream(c.frame, c.plan, cb_load_stream(streams, i), c.target, s_in, s_out, s_tq, lane);
        } else if constexpr (WHICH == CBW_ZSTD) {
            __shared__ __attribute__((aligned(16))) ZsState s_zs;
            if (c.codec != CB_CODEC_ZSTD) continue;
            cb_decode_zstd_stream(c.frame, c.plan, cb_load_stream(streams, i), c.target, &s_zs, lane);
        } else if constexpr (WHICH == CBW_ZLIB) {
            __shared__ __attribute__((aligned(16))) ZlState s_zl;
            if (c.codec != CB_CODEC_ZLIB) continue;
            cb_decode_zlib_stream(c.frame, c.plan, cb_load_stream(streams, i), c.target, &s_zl, lane);
        } else {
            __shared__ __attribute__((aligned(16))) uint8_t s_win[RG_PWIN + 128];
            __shared__ __attribute__((aligned(16))) uint8_t s_d[SY_IMG + 64];
            if (c.codec != (WHICH == CBW_BLZ ? CB_CODEC_BLOSCLZ : CB_CODEC_LZ4)) continue;
            cb_decode_stream<WHICH == CBW_BLZ ? RG_BLOSCLZ : RG_LZ4>(c.frame, c.plan, cb_load_stream(streams, i), c.target, WHICH == CBW_LZ4 && small_launched && c.small,
                                                                     s_win, s_tq, s_d, lane);
        }
    }
}

// a run-time kind (CBK_* / CBG_*: 0 .. 3) as a compile-time one: f(std::integral_constant<int, K>{}); anything else is the last kind
static_assert(CBK_COUNT == 4 && CBK_COPY == 3 && CBG_COUNT == 4 && CBG_BITUN4 == 3, "cb_with_kind's default is the last kind of either set");
template <class F>
static inline void cb_with_kind(int k, F &&f) {
    switch (k) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
    }
}
// The decoder launches of a space: the small decoder, LZ4, BloscLZ, zstd, zlib, each when an owner needs it, under the stage names of the family.
template <class SPACE>
static void cb_launch_streams(const SPACE &sp, const CbStream *streams, uint32_t nstreams, uint32_t any_small, uint32_t any_lz4, uint32_t any_blz, uint32_t any_zstd, uint32_t any_zlib,
                              uint32_t nsplit_all, const char *name_small, const char *name_lz4, const char *name_blz, const char *name_zstd, const char *name_zlib, hipStream_t s) {
    const CbSchedule S = cb_decode_schedule(nstreams, nsplit_all, any_small);
    auto launch = [&](auto which, uint32_t grid, const char *name) {
        hb_prof_begin(name, s);
        hipLaunchKernelGGL((k_cb_streams<SPACE, decltype(which)::value>), dim3(grid), dim3(64), 0, s, sp, streams, nstreams, (int)any_small, S.P);
        hb_prof_end(s);
    };
    if (any_small) launch(std::integral_constant<int, CBW_SMALL>{}, S.grid_small, name_small);
    if (any_lz4) launch(std::integral_constant<int, CBW_LZ4>{}, S.grid_lz4, name_lz4);      // (any owner can have stored streams: it runs next to the small one)
    if (any_blz) launch(std::integral_constant<int, CBW_BLZ>{}, S.grid_blz, name_blz);
    if (any_zstd) launch(std::integral_constant<int, CBW_ZSTD>{}, S.grid_blz, name_zstd);      // (no workspace of its own: the grid needs no cap)
    if (any_zlib) launch(std::integral_constant<int, CBW_ZLIB>{}, S.grid_blz, name_zlib);      // (the same)
}

// ---- what the launch code of the read batches shares (the getitem batch and cbx_launch below) ----
// a section of the one upload: the vector to its layout offset, unless it is empty; and a section of the workspace as the records it holds
template <class T>
static inline void cb_put(std::vector<uint8_t> &up, size_t at, const std::vector<T> &v) {
    if (!v.empty()) memcpy(up.data() + at, v.data(), v.size() * sizeof(T));
}
template <class T>
static inline T *cb_at(uint8_t *w, size_t at) { return (T *)(w + at); }
// One launch per kind that occurs among a gather's jobs: kind0 = where each kind's jobs start in the launch list (CBG_COUNT + 1 entries),
// kblocks / names = the kind's workgroup count and profile stage.  launch(K, k0, nk, blocks) gets the kind as a compile-time constant.
template <class LAUNCH>
static void cb_launch_kinds(const uint32_t *kind0, const uint32_t *kblocks, const char *const *names, hipStream_t s, LAUNCH &&launch) {
    for (int k = 0; k < CBG_COUNT; k++) {
        const uint32_t k0 = kind0[k], nk = kind0[k + 1] - k0, blocks = kblocks[k];
        if (!nk) continue;
        hb_prof_begin(names[k], s);
        cb_with_kind(k, [&](auto K) { launch(K, k0, nk, blocks); });      // (any other kind: CBG_BITUN4, the last)
        hb_prof_end(s);
    }
}

// ---- the per-block filters, undone ----
// (bodies with their workgroup index `bx` and grid size `gx`: the one-frame kernels pass blockIdx.x / gridDim.x, k_cbb_unfilter the workgroup's
// place among those of its frame)
// byte shuffle: block bytes [plane 0 | plane 1 | ...] -> elements; one thread per element (typesize 4 / 8: one store)
__device__ __forceinline__ void cb_unshuffle(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nbytes, uint32_t blocksize, uint32_t ts, uint32_t bx, uint32_t gx) {
    const uint32_t nblocks = (nbytes + blocksize - 1) / blocksize;
    const uint32_t per = blocksize / ts + 1u;                                          // threads per block: elements + one for the tail
    for (uint64_t i = (uint64_t)bx * blockDim.x + threadIdx.x; i < (uint64_t)nblocks * per; i += (uint64_t)gx * blockDim.x) {
        const uint32_t b = (uint32_t)(i / per), e = (uint32_t)(i % per);
        const uint32_t base = b * blocksize, bsize = nbytes - base < blocksize ? nbytes - base : blocksize, nel = bsize / ts;
        if (e < nel) {
            const uint8_t *s = src + base + e;
            uint8_t *d = dst + base + (size_t)e * ts;
            if (ts == 4u) { st4u(d, (uint32_t)s[0] | ((uint32_t)s[nel] << 8) | ((uint32_t)s[2u * nel] << 16) | ((uint32_t)s[3u * nel] << 24)); }
            else for (uint32_t j = 0; j < ts; j++) d[j] = s[(size_t)j * nel];
        } else if (e == nel) {
            for (uint32_t k = nel * ts; k < bsize; k++) dst[base + k] = src[base + k];   // the bytes behind the last whole element
        }
    }
}
__global__ void k_cb_unshuffle(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nbytes, uint32_t blocksize, uint32_t ts) {
    cb_unshuffle(dst, src, nbytes, blocksize, ts, blockIdx.x, gridDim.x);
}
// bit shuffle: one thread per group of 8 elements
__device__ __forceinline__ void cb_bitunshuffle(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nbytes, uint32_t blocksize, uint32_t ts, uint32_t bx, uint32_t gx) {
    const uint32_t nblocks = (nbytes + blocksize - 1) / blocksize;
    const uint32_t per = blocksize / (8u * ts) + 1u;
    for (uint64_t i = (uint64_t)bx * blockDim.x + threadIdx.x; i < (uint64_t)nblocks * per; i += (uint64_t)gx * blockDim.x) {
        const uint32_t b = (uint32_t)(i / per), g = (uint32_t)(i % per);
        const uint32_t base = b * blocksize, bsize = nbytes - base < blocksize ? nbytes - base : blocksize, nel = bsize / ts;
        if (nel % 8u != 0u) {                                                           // not filtered at all: the threads of the block copy it
            for (uint32_t k = g; k < bsize; k += per) dst[base + k] = src[base + k];
            continue;
        }
        const uint32_t ng = nel / 8u;                                                   // bytes per bit row
        if (g < ng) {
            for (uint32_t j = 0; j < ts; j++) {
                uint64_t x = 0;                                                         // byte k = row 8 j + k, elements 8 g .. 8 g + 7
                for (uint32_t k = 0; k < 8u; k++) x |= (uint64_t)src[base + (size_t)(8u * j + k) * ng + g] << (8u * k);
                // 8 x 8 bit transpose: out byte i, bit k = in byte k, bit i
                uint64_t t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull; x ^= t ^ (t << 7);
                t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
                t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
                for (uint32_t e = 0; e < 8u; e++) dst[base + (size_t)(8u * g + e) * ts + j] = (uint8_t)(x >> (8u * e));
            }
        } else if (g == ng) {
            for (uint32_t k = nel * ts; k < bsize; k++) dst[base + k] = src[base + k];
        }
    }
}
__global__ void k_cb_bitunshuffle(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nbytes, uint32_t blocksize, uint32_t ts) {
    cb_bitunshuffle(dst, src, nbytes, blocksize, ts, blockIdx.x, gridDim.x);
}

// 8 x 8 bit transpose: out byte i, bit k = in byte k, bit i
__device__ __forceinline__ uint64_t cb_transpose8(uint64_t x) {
    uint64_t t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull; x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
    return x;
}
// typesize 4, whole blocks of a multiple of 32 elements (what every writer's block size is): one thread per 32 elements -- 32 dword
// loads (4 groups of every bit row at once), 8 x 16-byte stores -- instead of one byte per access
// one work item of the inverse: 32 elements, group q of 4 bytes of every bit row of the block at `base` (ng = bytes per bit row)
__device__ __forceinline__ void cb_bitunshuffle4_item(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, size_t base, uint32_t ng, uint32_t q) {
        uint64_t x[4][4];                                                   // [byte j][group]: byte e = byte j of element 8 (4 q + group) + e
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t r[8];
#pragma unroll
            for (int k = 0; k < 8; k++) r[k] = ld4u(src + base + (size_t)(8 * j + k) * ng + 4u * q);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                uint64_t v = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) v |= (uint64_t)((r[k] >> (8 * g)) & 255u) << (8 * k);
                x[j][g] = cb_transpose8(v);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
            uint32_t w[8];
#pragma unroll
            for (int e = 0; e < 8; e++)
                w[e] = (uint32_t)((x[0][g] >> (8 * e)) & 255u) | ((uint32_t)((x[1][g] >> (8 * e)) & 255u) << 8) |
                       ((uint32_t)((x[2][g] >> (8 * e)) & 255u) << 16) | ((uint32_t)((x[3][g] >> (8 * e)) & 255u) << 24);
            u32x4 a, bb; a.x = w[0]; a.y = w[1]; a.z = w[2]; a.w = w[3]; bb.x = w[4]; bb.y = w[5]; bb.z = w[6]; bb.w = w[7];
            st16u(dst + base + (size_t)(32u * q + 8u * g) * 4u, a);
            st16u(dst + base + (size_t)(32u * q + 8u * g) * 4u + 16u, bb);
        }
}
template <bool FWD>
__global__ void k_cb_bitshuffle4_fast(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nfull, uint32_t blocksize) {
    const uint32_t ng = blocksize / 32u, per = ng / 4u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (uint64_t)nfull * per; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t b = (uint32_t)(i / per), q = (uint32_t)(i % per);
        const size_t base = (size_t)b * blocksize;
        if (!FWD) cb_bitunshuffle4_item(dst, src, base, ng, q);
        else {
            uint32_t r[4][8];                                                   // [byte j][bit k]: 4 bytes = groups 4 q .. 4 q + 3 of row 8 j + k
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 8; k++) r[j][k] = 0;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const u32x4 a = ld16u(src + base + (size_t)(32u * q + 8u * g) * 4u), bb = ld16u(src + base + (size_t)(32u * q + 8u * g) * 4u + 16u);
                const uint32_t w[8] = {a.x, a.y, a.z, a.w, bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint64_t v = 0;
#pragma unroll
                    for (int e = 0; e < 8; e++) v |= (uint64_t)((w[e] >> (8 * j)) & 255u) << (8 * e);
                    v = cb_transpose8(v);                                       // byte k = bit k of byte j of the 8 elements
#pragma unroll
                    for (int k = 0; k < 8; k++) r[j][k] |= (uint32_t)((v >> (8 * k)) & 255u) << (8 * g);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 8; k++) st4u(dst + base + (size_t)(8 * j + k) * ng + 4u * q, r[j][k]);
        }
    }
}
// one work item of the forward direction for k_cbeb_filter: the loop body of k_cb_bitshuffle4_fast<true> once more -- that kernel keeps its own
// copy, because calling a function from its loop costs it 24 VGPRs (66 -> 90, occupancy 7 -> 5)
__device__ __forceinline__ void cb_bitshuffle4_item(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, size_t base, uint32_t ng, uint32_t q) {
            uint32_t r[4][8];                                                   // [byte j][bit k]: 4 bytes = groups 4 q .. 4 q + 3 of row 8 j + k
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 8; k++) r[j][k] = 0;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const u32x4 a = ld16u(src + base + (size_t)(32u * q + 8u * g) * 4u), bb = ld16u(src + base + (size_t)(32u * q + 8u * g) * 4u + 16u);
                const uint32_t w[8] = {a.x, a.y, a.z, a.w, bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint64_t v = 0;
#pragma unroll
                    for (int e = 0; e < 8; e++) v |= (uint64_t)((w[e] >> (8 * j)) & 255u) << (8 * e);
                    v = cb_transpose8(v);                                       // byte k = bit k of byte j of the 8 elements
#pragma unroll
                    for (int k = 0; k < 8; k++) r[j][k] |= (uint32_t)((v >> (8 * k)) & 255u) << (8 * g);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 8; k++) st4u(dst + base + (size_t)(8 * j + k) * ng + 4u * q, r[j][k]);
}
// either direction over the workgroups [0, gx) of one frame (k_cbb_unfilter, k_cbeb_filter)
__device__ __forceinline__ void cb_bitshuffle4_fast(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nfull, uint32_t blocksize, uint32_t bx, uint32_t gx) {
    const uint32_t ng = blocksize / 32u, per = ng / 4u;
    for (uint64_t i = (uint64_t)bx * blockDim.x + threadIdx.x; i < (uint64_t)nfull * per; i += (uint64_t)gx * blockDim.x)
        cb_bitshuffle4_item(dst, src, (size_t)(uint32_t)(i / per) * blocksize, ng, (uint32_t)(i % per));
}
__device__ __forceinline__ void cb_bitunshuffle4_fast(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nfull, uint32_t blocksize, uint32_t bx, uint32_t gx) {
    const uint32_t ng = blocksize / 32u, per = ng / 4u;
    for (uint64_t i = (uint64_t)bx * blockDim.x + threadIdx.x; i < (uint64_t)nfull * per; i += (uint64_t)gx * blockDim.x)
        cb_bitunshuffle4_item(dst, src, (size_t)(uint32_t)(i / per) * blocksize, ng, (uint32_t)(i % per));
}

__device__ __forceinline__ void cb_result(const CbPlan *plan, hb_result *result, uint64_t nbytes) {
    result->flags = 1; result->total_bytes = nbytes; result->reserved = 0;
    if (plan->fail) { result->status = HB_ERR_DECOMPRESSION_FAILED; result->bytes = 0; }
    else { result->status = HB_OK; result->bytes = nbytes; }
}
__global__ void k_cb_result(const CbPlan *plan, hb_result *result, uint64_t nbytes) { cb_result(plan, result, nbytes); }
// a job or a frame the host refused: its status, nothing decoded
__device__ __forceinline__ void cb_refused_result(hb_result *r, int status) { r->status = status; r->flags = 0; r->bytes = 0; r->total_bytes = 0; r->reserved = 0; }
__global__ void k_cb_init(CbPlan *plan) { plan->fail = 0; }

// ---- batches (hb_cblosc_decompress_frames_batch_device): many frames through ONE set of launches.  Blocks and streams are as independent
// across frames as inside one, so the same bodies run over flat spaces; the records, prefixes and kinds are hb_cblosc_batch.h's. ----
// one thread per block of the flat block space
__global__ __launch_bounds__(64) void k_cbb_plan(const CbbFrame *__restrict__ frames, CbPlan *plans, const uint32_t *__restrict__ blk0, uint32_t nframes,
                                                  uint32_t nblocks, CbStream *streams) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x;
    if (x >= nblocks) return;
    const uint32_t k = hb_owner(blk0, nframes, x);
    const CbbFrame &F = frames[k];
    cb_plan_block(F.frame, F.nbytes, F.blocksize, F.cbytes, F.typesize, F.flags, plans + k, streams + F.stream0, F.b0, x - blk0[k]);
}

// one launch per kind that occurs: ufrm / ublk = the frames of this kind and the prefix of their workgroup counts (every frame has at least one).
// CBK_COPY is the memcpyed frames' copy: one wavefront per 4 KiB piece.
template <int KIND>
__global__ __launch_bounds__(256) void k_cbb_unfilter(const CbbFrame *__restrict__ frames, const uint32_t *__restrict__ ufrm, const uint32_t *__restrict__ ublk,
                                                       uint32_t nkind, uint8_t *work) {
    const uint32_t i = hb_owner(ublk, nkind, blockIdx.x);
    const CbbFrame &F = frames[ufrm[i]];
    const uint32_t bx = blockIdx.x - ublk[i], gx = F.ngrid;
    uint8_t *dst = F.dst;
    if constexpr (KIND == CBK_COPY) {
        const uint32_t off = (bx * 4u + (threadIdx.x >> 6)) * HB_CHUNK;        // (ngrid = ceil(nbytes / 16 KiB): every piece has its wavefront)
        if (off < F.nbytes) wave_copy_g2g(dst + off, F.frame + 16 + off, F.nbytes - off < HB_CHUNK ? F.nbytes - off : HB_CHUNK, (int)(threadIdx.x & 63u));
    } else {
        const uint8_t *src = work + F.stage_off;
        if constexpr (KIND == CBK_UNSHUFFLE) cb_unshuffle(dst, src, F.nbytes, F.blocksize, F.typesize, bx, gx);
        else if constexpr (KIND == CBK_BITUN) cb_bitunshuffle(dst, src, F.nbytes, F.blocksize, F.typesize, bx, gx);
        else {
            const uint32_t nfull = F.nbytes / F.blocksize;
            if (bx < F.nfast) cb_bitunshuffle4_fast(dst, src, nfull, F.blocksize, bx, F.nfast);
            else {                                                             // the last, shorter block the plain way
                const size_t done = (size_t)nfull * F.blocksize;
                cb_bitunshuffle(dst + done, src + done, F.nbytes - (uint32_t)done, F.blocksize, F.typesize, bx - F.nfast, gx - F.nfast);
            }
        }
    }
}

// one thread per frame: what the host decided, or k_cb_result's record
__global__ __launch_bounds__(64) void k_cbb_finish(const CbbFrame *__restrict__ frames, const CbPlan *plans, hb_result *results, uint32_t nframes) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= nframes) return;
    const CbbFrame &F = frames[k];
    hb_result *r = results + k;
    if (F.mode == CBB_REFUSED) { cb_refused_result(r, F.status); return; }
    cb_result(plans + k, r, (uint64_t)F.nbytes);
}

// ---- batched getitem (hb_cblosc_getitem_frames_batch_device): many item ranges of many frames through ONE set of launches.  What is planned and
// decoded is the DISTINCT (frame, block) pairs the jobs cover (hb_cblosc_getitem_batch.h: one CbgBlock each, with a CbPlan and a staged copy of
// its own), whole and once; a gather per job then un-filters exactly the job's bytes out of the staged, still filtered blocks. ----
// one thread per block record
__global__ __launch_bounds__(64) void k_cbg_plan(const CbgFrame *__restrict__ frames, const CbgBlock *__restrict__ blocks, CbPlan *plans, uint32_t nblk, CbStream *streams) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x;
    if (x >= nblk) return;
    const CbgBlock &K = blocks[x];
    const CbgFrame &F = frames[K.frame];
    cb_plan_block(F.frame, F.nbytes, F.blocksize, F.cbytes, F.typesize, F.flags, plans + x, streams + K.stream0, K.b, 0u, true);
}
// ---- the clipped un-filter: byte p of the frame's decoded bytes out of the staged blocks.  `look(b)` is the record of block number b: the
// ranges' jobs have consecutive records (CbgSeqLookup), the boxes' a list of the blocks they touch (CbxLookup).  The plain body: the edges of
// every range, and every shape the wide bodies below leave alone. ----
struct CbgSeqLookup {
    const CbgBlock *__restrict__ first; uint32_t b_lo;                        // the job's first record and its block number
    __device__ __forceinline__ const CbgBlock &operator()(uint32_t b) const { return first[b - b_lo]; }
};
template <int KIND, class LOOK>
__device__ __forceinline__ uint8_t cbg_byte(const CbgFrame &F, const LOOK &look, const uint8_t *__restrict__ work, uint32_t p) {
    if (KIND == CBG_COPY && F.memcpyed) return F.frame[16u + (size_t)p];
    const uint32_t b = p / F.blocksize, q = p - b * F.blocksize;
    const CbgBlock &K = look(b);
    const uint8_t *s = work + K.stage_off;
    if (KIND == CBG_COPY) return s[q];
    const uint32_t ts = F.typesize, nel = K.bsize / ts;
    if (q >= nel * ts) return s[q];                                            // the bytes behind the last whole element
    const uint32_t e = q / ts, j = q - e * ts;
    if (KIND == CBG_UNSHUFFLE) return s[j * nel + e];
    if (nel & 7u) return s[q];                                                 // not a multiple of 8 elements: the block was not filtered
    const uint32_t ng = nel >> 3, g = e >> 3;
    uint64_t x = 0;                                                            // byte k = row 8 j + k, elements 8 g .. 8 g + 7
    for (uint32_t k = 0; k < 8u; k++) x |= (uint64_t)s[(size_t)(8u * j + k) * ng + g] << (8u * k);
    return (uint8_t)(cb_transpose8(x) >> (8u * (e & 7u)));
}
// 16 bytes = 16 / TS whole elements starting with element e of a byte-shuffled block of nel elements
template <uint32_t TS>
__device__ __forceinline__ u32x4 cbg_unshuffle16(const uint8_t *__restrict__ s, uint32_t nel, uint32_t e) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < TS; j++)
#pragma unroll
        for (uint32_t c = 0; c < 16u / TS; c++) {
            const uint32_t i = c * TS + j;
            w[i >> 2] |= (uint32_t)s[(size_t)j * nel + e + c] << (8u * (i & 3u));
        }
    u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    return v;
}
// the 8 * ts bytes of a whole group of 8 elements at byte q of a bit-shuffled block (false: not such a group -- the plain body has it)
__device__ __forceinline__ bool cbg_bitun_group(uint8_t *__restrict__ d, const uint8_t *__restrict__ s, uint32_t bsize, uint32_t ts, uint32_t q) {
    const uint32_t nel = bsize / ts, e = q / ts;
    if ((nel & 7u) || e * ts != q || (e & 7u) || e + 8u > nel) return false;
    const uint32_t ng = nel >> 3, g = e >> 3;
    for (uint32_t j = 0; j < ts; j++) {
        uint64_t x = 0;
        for (uint32_t k = 0; k < 8u; k++) x |= (uint64_t)s[(size_t)(8u * j + k) * ng + g] << (8u * k);
        x = cb_transpose8(x);
        for (uint32_t k = 0; k < 8u; k++) d[k * ts + j] = (uint8_t)(x >> (8u * k));
    }
    return true;
}
// One gather unit: bytes [lo, hi) of the frame's decoded bytes to d.  A unit is cbg_unit_bytes() bytes counted from the start of the FRAME (so
// that it does not straddle a block, a group or an item where the block size allows it), clipped to the range or the row it belongs to: a
// whole unit of a fitting shape takes the wide body, everything else the plain one.  Destinations have any alignment.
template <int KIND, class LOOK>
__device__ __forceinline__ void cbg_unit(const CbgFrame &F, const LOOK &look, const uint8_t *__restrict__ work, uint32_t lo, uint32_t hi, uint8_t *__restrict__ d) {
    const uint32_t ts = F.typesize, bs = F.blocksize, U = cbg_unit_bytes(KIND, ts);
    if (hi - lo == U) {                                                        // a whole unit
        if (KIND == CBG_COPY && F.memcpyed) { st16u(d, ld16u(F.frame + 16u + (size_t)lo)); return; }
        const uint32_t b = lo / bs, q = lo - b * bs;
        const CbgBlock &K = look(b);
        const uint8_t *s = work + K.stage_off;
        if (KIND == CBG_COPY) {
            if (q + 16u <= K.bsize) { st16u(d, ld16u(s + q)); return; }
        } else if (KIND == CBG_UNSHUFFLE) {
            const uint32_t nel = K.bsize / ts, e = q / ts;
            if (e * ts == q && q + 16u <= nel * ts) {
                if (ts == 2u) { st16u(d, cbg_unshuffle16<2>(s, nel, e)); return; }
                if (ts == 4u) { st16u(d, cbg_unshuffle16<4>(s, nel, e)); return; }
                if (ts == 8u) { st16u(d, cbg_unshuffle16<8>(s, nel, e)); return; }
                if (ts == 16u) { st16u(d, cbg_unshuffle16<16>(s, nel, e)); return; }
            }
        } else if (KIND == CBG_BITUN) {
            if (q + U <= K.bsize && cbg_bitun_group(d, s, K.bsize, ts, q)) return;
        } else {
            // typesize 4, block size a multiple of 512: q is a multiple of 128.  A whole block takes cb_bitunshuffle4_item's arithmetic for item
            // q / 128 (32 elements: 32 dword loads, 8 x 16-byte stores); the last, shorter block goes group by group
            if (K.bsize == bs) { cb_bitunshuffle4_item(d, s + (q >> 5), 0, bs >> 5, 0u); return; }
            if (q + 128u <= K.bsize) {
                for (uint32_t g = 0; g < 4u; g++)
                    if (!cbg_bitun_group(d + 32u * g, s, K.bsize, 4u, q + 32u * g))
                        for (uint32_t k = 0; k < 32u; k++) d[32u * g + k] = cbg_byte<KIND>(F, look, work, lo + 32u * g + k);
                return;
            }
        }
    }
    for (uint32_t p = lo; p < hi; p++) d[p - lo] = cbg_byte<KIND>(F, look, work, p);
}
// One launch per kind that occurs: gjob / gblk = the jobs of this kind and the prefix of their workgroup counts.  A thread has one unit
// (cbg_unit) clipped to the job's range.  Nothing is written outside [0, nitems * typesize) of the job's destination, and nothing at all when
// one of the job's blocks failed.
template <int KIND>
__global__ __launch_bounds__(256) void k_cbg_gather(const CbgFrame *__restrict__ frames, const CbgJob *__restrict__ jobs, const CbgBlock *__restrict__ blocks,
                                                     const CbPlan *__restrict__ plans, const uint32_t *__restrict__ gjob, const uint32_t *__restrict__ gblk, uint32_t nkind,
                                                     const uint8_t *__restrict__ work) {
    const uint32_t i = hb_owner(gblk, nkind, blockIdx.x);
    const CbgJob &J = jobs[gjob[i]];
    const CbgFrame &F = frames[J.frame];
    int bad = 0;
    for (uint32_t k = threadIdx.x; k < J.nb; k += 256u) bad |= plans[J.blk0 + k].fail != 0u;
    if (__syncthreads_or(bad)) return;
    const uint32_t U = cbg_unit_bytes(KIND, F.typesize);
    const uint64_t at = ((uint64_t)J.unit0 + (uint64_t)(blockIdx.x - gblk[i]) * 256u + threadIdx.x) * U, end = J.off + J.bytes;
    if (at >= end) return;
    const uint32_t lo = (uint32_t)(at > J.off ? at : J.off), hi = (uint32_t)(at + U < end ? at + U : end);      // (end <= nbytes < 2^32)
    const CbgSeqLookup look{blocks + J.blk0, (KIND == CBG_COPY && F.memcpyed) ? 0u : (uint32_t)(J.off / F.blocksize)};
    cbg_unit<KIND>(F, look, work, lo, hi, J.dst + (lo - J.off));
}

// One thread per job: what the host decided, or k_cb_result's record from the OR of the fail words of the job's `nrec` block records, the k-th
// of which is plan rec(J, k).  The body of k_cbg_finish (consecutive records) and k_cbx_finish (the touch list).
template <class JOB, class REC>
__device__ __forceinline__ void cb_finish_jobs(const JOB *__restrict__ jobs, const CbPlan *__restrict__ plans, hb_result *results, uint32_t njobs, uint32_t JOB::*nrec, REC rec) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= njobs) return;
    const JOB &J = jobs[j];
    hb_result *r = results + j;
    if (J.status) { cb_refused_result(r, J.status); return; }
    CbPlan p; p.fail = 0u;
    for (uint32_t k = 0; k < J.*nrec; k++) p.fail |= plans[rec(J, k)].fail;
    cb_result(&p, r, J.bytes);
}
__global__ __launch_bounds__(64) void k_cbg_finish(const CbgJob *__restrict__ jobs, const CbPlan *__restrict__ plans, hb_result *results, uint32_t njobs) {
    cb_finish_jobs(jobs, plans, results, njobs, &CbgJob::nb, [](const CbgJob &J, uint32_t k) { return J.blk0 + k; });
}

// ---- batched box reads (hb_cblosc_getbox_frames_batch_device; the host side and the index arithmetic are hb_cblosc_box_batch.h).  The plan and
// the decoders above run over the distinct block records as they are; the gather walks a job's rows by arithmetic. ----
struct CbxLookup {
    const CbgBlock *__restrict__ blocks; const CbxTouch *__restrict__ tl; uint32_t ntl, b_lo, dense;      // the job's touch list
    __device__ __forceinline__ const CbgBlock &operator()(uint32_t b) const { return blocks[tl[cbx_find(tl, ntl, b_lo, dense, b)].rec]; }
};
// How the four N-d gather kernels below open: gjob / gblk = the jobs of the launch and the prefix of their workgroup counts.  The workgroup finds
// its job (number i of the launch: its row record, where the launch has them, is rows[i]) and its place wl among the job's workgroups, ORs the fail
// words of the blocks the job touches and is not `live` -- the whole workgroup, before any store -- if one is set.  The records are the kernels'
// own `const __restrict__` arguments handed through: inlined, they are read with scalar loads as before (CB_RO above says what else costs).
struct CbxWg {
    bool live; const CbxJob &J; const CbgFrame &F; uint32_t i, wl; CbxLookup look;
};
__device__ __forceinline__ CbxWg cbx_enter(const CbgFrame *__restrict__ frames, const CbxJob *__restrict__ jobs, const CbgBlock *__restrict__ blocks, const CbPlan *__restrict__ plans,
                                           const CbxTouch *__restrict__ touch, const uint32_t *__restrict__ gjob, const uint32_t *__restrict__ gblk, uint32_t nkind) {
    const uint32_t i = hb_owner(gblk, nkind, blockIdx.x);
    const CbxJob &J = jobs[gjob[i]];
    const CbxTouch *tl = touch + J.tl0;
    int bad = 0;
    for (uint32_t k = threadIdx.x; k < J.ntl; k += 256u) bad |= plans[tl[k].rec].fail != 0u;
    const bool live = !__syncthreads_or(bad);
    return CbxWg{live, J, frames[J.frame], i, blockIdx.x - gblk[i], CbxLookup{blocks, tl, J.ntl, J.b_lo, J.dense}};
}
// One launch per kind that occurs, over a workgroup prefix per job.  A job's thread space is rows x units per row (cbx_thread: whole rows to a
// workgroup where rows are short, several workgroups to a row where they are long; the divisions are multiplications by reciprocals the host
// put into the record).
template <int KIND>
__global__ __launch_bounds__(256) void k_cbx_gather(const CbgFrame *__restrict__ frames, const CbxJob *__restrict__ jobs, const CbgBlock *__restrict__ blocks,
                                                     const CbPlan *__restrict__ plans, const CbxTouch *__restrict__ touch, const uint32_t *__restrict__ gjob,
                                                     const uint32_t *__restrict__ gblk, uint32_t nkind, const uint8_t *__restrict__ work) {
    const CbxWg W = cbx_enter(frames, jobs, blocks, plans, touch, gjob, gblk, nkind);
    if (!W.live) return;
    uint32_t lo, hi;
    uint64_t doff;
    if (!cbx_thread(W.J, cbg_unit_bytes(KIND, W.F.typesize), W.wl, threadIdx.x, lo, hi, doff)) return;
    cbg_unit<KIND>(W.F, W.look, work, lo, hi, W.J.dst + doff);
}
// ---- rows of items: the stepped rows of the slice batch (hb_cblosc_getslice_frames_batch_device; hb_cblosc_slice_batch.h) and the listed or
// stepped rows of the index batch below.  A unit is 16 bytes of the row's destination: items that lie at(0), at(1) ... bytes behind byte p of
// the frame's decoded bytes, `at` being one of two by-value policies.  Which one is the kernel's choice at compile time: the stepped gather
// has no table to test for. ----
struct CbsStepped {                                                            // a stepped row from its first item of the unit on: i * istr
    uint32_t istr;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return i * istr; }
};
struct CbiListed {                                                             // a row of the index batch from its start on, the unit's first item being `it`: cbi_item
    const uint32_t *__restrict__ rt; uint32_t istr, it;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return cbi_item(rt, istr, it + i); }
};
// 16 bytes = 16 / TS items.  An item that lies whole inside the whole elements of its block is read where it is staged (a byte-shuffled block
// plane by plane); one that straddles two blocks or lies behind a block's last whole element goes byte by byte through cbg_byte.  Neighbouring
// items usually share a block: its record is looked up once.
template <int KIND, uint32_t TS, class LOOK, class AT>
__device__ __forceinline__ u32x4 cbr_items16(const CbgFrame &F, const LOOK &look, const uint8_t *__restrict__ work, uint32_t p, const AT at) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const uint32_t bs = F.blocksize;
    const bool direct = KIND == CBG_COPY && F.memcpyed;
    uint32_t cur = ~0u, bsize = 0u, nel = 0u;
    const uint8_t *s = nullptr;
#pragma unroll
    for (uint32_t c = 0; c < 16u / TS; c++) {
        const uint32_t pc = p + at(c);
        uint32_t q = 0u, e = 0u;
        bool whole = direct;
        if (!direct) {
            const uint32_t b = pc / bs;
            q = pc - b * bs;
            if (b != cur) { const CbgBlock &K = look(b); s = work + K.stage_off; bsize = K.bsize; nel = bsize / TS; cur = b; }
            if (KIND == CBG_COPY) whole = q + TS <= bsize;
            else { e = q / TS; whole = e * TS == q && e < nel; }
        }
#pragma unroll
        for (uint32_t j = 0; j < TS; j++) {
            const uint32_t i = c * TS + j;
            const uint8_t v = direct ? F.frame[16u + (size_t)pc + j] : !whole ? cbg_byte<KIND>(F, look, work, pc + j) : KIND == CBG_COPY ? s[q + j] : s[(size_t)j * nel + e];
            w[i >> 2] |= (uint32_t)v << (8u * (i & 3u));
        }
    }
    u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    return v;
}
// One unit of a row: `cnt` items to d, packed.  16 bytes of whole items of a copied or byte-shuffled frame are assembled in registers and stored
// at once (d has any alignment); the plain body has the row tails, the other typesizes and both bit-shuffle kinds -- through cbg_byte, which
// reads a bit-shuffled block the same way for CBG_BITUN and CBG_BITUN4.
template <int KIND, class LOOK, class AT>
__device__ __forceinline__ void cbr_unit(const CbgFrame &F, const LOOK &look, const uint8_t *__restrict__ work, uint32_t p, const AT at, uint32_t cnt, uint8_t *__restrict__ d) {
    const uint32_t ts = F.typesize;
    if ((KIND == CBG_COPY || KIND == CBG_UNSHUFFLE) && cnt * ts == 16u) {
        if (ts == 1u && KIND == CBG_COPY) { st16u(d, cbr_items16<KIND, 1>(F, look, work, p, at)); return; }      // (one byte is never shuffled)
        if (ts == 2u) { st16u(d, cbr_items16<KIND, 2>(F, look, work, p, at)); return; }
        if (ts == 4u) { st16u(d, cbr_items16<KIND, 4>(F, look, work, p, at)); return; }
        if (ts == 8u) { st16u(d, cbr_items16<KIND, 8>(F, look, work, p, at)); return; }
        if (ts == 16u) { st16u(d, cbr_items16<KIND, 16>(F, look, work, p, at)); return; }
    }
    for (uint32_t c = 0; c < cnt; c++) {
        const uint32_t pc = p + at(c);
        for (uint32_t j = 0; j < ts; j++) d[c * ts + j] = cbg_byte<KIND>(F, look, work, pc + j);
    }
}
// The kind an items gather is launched with.  KIND reaches cbr_unit alone -- cbs_thread and cbi_thread_items do not see it -- and there the two
// bit-shuffle kinds have the plain body only, in which cbg_byte tests nothing but KIND == CBG_COPY and KIND == CBG_UNSHUFFLE: the CBG_BITUN4
// instantiation would be the CBG_BITUN one once more (it was: the same instructions, 35 VGPRs each).  So jobs of kind CBG_BITUN4 run the CBG_BITUN
// instantiation, under their own stage name; the host sorts the jobs into four kinds as for every other gather.
static constexpr int cbr_items_kind(int kind) { return kind == CBG_BITUN4 ? CBG_BITUN : kind; }
// The slice batch's gather: one launch per kind that occurs among the jobs with stepped rows; gjob / gblk / rows are those jobs in launch
// order.  A job's thread space is rows x units per row (cbs_thread).  Everything but this gather is the box batch's.
template <int KIND>
__global__ __launch_bounds__(256) void k_cbs_gather(const CbgFrame *__restrict__ frames, const CbxJob *__restrict__ jobs, const CbsRow *__restrict__ rows,
                                                     const CbgBlock *__restrict__ blocks, const CbPlan *__restrict__ plans, const CbxTouch *__restrict__ touch,
                                                     const uint32_t *__restrict__ gjob, const uint32_t *__restrict__ gblk, uint32_t nkind, const uint8_t *__restrict__ work) {
    const CbxWg W = cbx_enter(frames, jobs, blocks, plans, touch, gjob, gblk, nkind);
    if (!W.live) return;
    const CbsRow R = rows[W.i];
    uint32_t it0, cnt, roff;
    uint64_t doff;
    if (!cbs_thread(W.J, R, W.F.typesize, W.wl, threadIdx.x, it0, cnt, roff, doff)) return;
    cbr_unit<KIND>(W.F, W.look, work, roff + it0 * R.istr, CbsStepped{R.istr}, cnt, W.J.dst + doff);
}
// ---- batched index-list reads (hb_cblosc_getindex_frames_batch_device; hb_cblosc_index_batch.h): the jobs in which a dimension takes its
// indices from a list.  Everything but the two gathers is the box batch's.  `tab` is the batch's table section: byte offsets, index * (chunk
// stride), in the caller's order. ----
// The rows gather: the row is a plain run, an outer dimension has a list.  A thread has one frame-aligned unit of a row (cbi_thread_rows) and
// the wide bodies of cbg_unit; only the row's offset comes from tables.
template <int KIND>
__global__ __launch_bounds__(256) void k_cbi_gather_rows(const CbgFrame *__restrict__ frames, const CbxJob *__restrict__ jobs, const CbiRow *__restrict__ rows,
                                                          const CbgBlock *__restrict__ blocks, const CbPlan *__restrict__ plans, const CbxTouch *__restrict__ touch,
                                                          const uint32_t *__restrict__ tab, const uint32_t *__restrict__ gjob, const uint32_t *__restrict__ gblk,
                                                          uint32_t nkind, const uint8_t *__restrict__ work) {
    const CbxWg W = cbx_enter(frames, jobs, blocks, plans, touch, gjob, gblk, nkind);
    if (!W.live) return;
    uint32_t lo, hi;
    uint64_t doff;
    if (!cbi_thread_rows(W.J, rows[W.i], tab, cbg_unit_bytes(KIND, W.F.typesize), W.wl, threadIdx.x, lo, hi, doff)) return;
    cbg_unit<KIND>(W.F, W.look, work, lo, hi, W.J.dst + doff);
}
// The items gather: the row has a list, or it is stepped while an outer dimension has one.  A thread has 16 bytes of the row's destination
// (cbi_thread_items) and reads each item's offset from the row's table, or by the row's step.
template <int KIND>
__global__ __launch_bounds__(256) void k_cbi_gather_items(const CbgFrame *__restrict__ frames, const CbxJob *__restrict__ jobs, const CbiRow *__restrict__ rows,
                                                           const CbgBlock *__restrict__ blocks, const CbPlan *__restrict__ plans, const CbxTouch *__restrict__ touch,
                                                           const uint32_t *__restrict__ tab, const uint32_t *__restrict__ gjob, const uint32_t *__restrict__ gblk,
                                                           uint32_t nkind, const uint8_t *__restrict__ work) {
    const CbxWg W = cbx_enter(frames, jobs, blocks, plans, touch, gjob, gblk, nkind);
    if (!W.live) return;
    const CbiRow R = rows[W.i];
    uint32_t it0, cnt, roff;
    uint64_t doff;
    if (!cbi_thread_items(W.J, R, tab, W.F.typesize, W.wl, threadIdx.x, it0, cnt, roff, doff)) return;
    cbr_unit<KIND>(W.F, W.look, work, roff, CbiListed{R.tab[3] != CBI_NONE ? tab + R.tab[3] : nullptr, R.istr, it0}, cnt, W.J.dst + doff);
}
// ---- batched point reads (hb_cblosc_getpoints_frames_batch_device; hb_cblosc_point_batch.h): a job is a run of the batch's point table, one
// entry per item -- where it starts in the frame's decoded bytes, where it goes in the job's destination.  Everything but this gather is the box
// batch's. ----
// One item of TS bytes at byte p of the frame's decoded bytes, in registers: an item that lies whole inside the whole elements of its block is
// read where it is staged (a byte-shuffled block plane by plane, TS byte loads at j * nel + e) after ONE lookup of its block; one that straddles
// two blocks or lies behind a block's last whole element goes byte by byte through cbg_byte, which looks up the block of every byte.
template <int KIND, uint32_t TS, class LOOK>
__device__ __forceinline__ void cbp_item_wide(const CbgFrame &F, const LOOK &look, const uint8_t *__restrict__ work, uint32_t p, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    const bool direct = KIND == CBG_COPY && F.memcpyed;
    const uint8_t *s = nullptr;
    uint32_t q = 0u, e = 0u, nel = 0u;
    bool whole = direct;
    if (!direct) {
        const uint32_t bs = F.blocksize, b = p / bs;
        q = p - b * bs;
        const CbgBlock &K = look(b);
        s = work + K.stage_off;
        nel = K.bsize / TS;
        if (KIND == CBG_COPY) whole = q + TS <= K.bsize;
        else { e = q / TS; whole = e * TS == q && e < nel; }
    }
#pragma unroll
    for (uint32_t j = 0; j < TS; j++) {
        const uint8_t v = direct ? F.frame[16u + (size_t)p + j] : !whole ? cbg_byte<KIND>(F, look, work, p + j) : KIND == CBG_COPY ? s[q + j] : s[(size_t)j * nel + e];
        w[j >> 2] |= (uint32_t)v << (8u * (j & 3u));
    }
}
// One point: the item at byte p to d, which has any alignment.  Typesizes 1, 2, 4, 8 and 16 of a copied or byte-shuffled frame are written with
// ONE store of the item's size; every other typesize and both bit-shuffle kinds go byte by byte through cbg_byte.
template <int KIND, class LOOK>
__device__ __forceinline__ void cbp_item(const CbgFrame &F, const LOOK &look, const uint8_t *__restrict__ work, uint32_t p, uint8_t *__restrict__ d) {
    const uint32_t ts = F.typesize;
    if (KIND == CBG_COPY || KIND == CBG_UNSHUFFLE) {
        uint32_t w[4];
        if (ts == 1u && KIND == CBG_COPY) { cbp_item_wide<KIND, 1>(F, look, work, p, w); d[0] = (uint8_t)w[0]; return; }      // (one byte is never shuffled)
        if (ts == 2u) { cbp_item_wide<KIND, 2>(F, look, work, p, w); ((hb_u16u *)d)->v = (uint16_t)w[0]; return; }
        if (ts == 4u) { cbp_item_wide<KIND, 4>(F, look, work, p, w); st4u(d, w[0]); return; }
        if (ts == 8u) { cbp_item_wide<KIND, 8>(F, look, work, p, w); st8u(d, (uint64_t)w[0] | ((uint64_t)w[1] << 32)); return; }
        if (ts == 16u) { cbp_item_wide<KIND, 16>(F, look, work, p, w); u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3]; st16u(d, v); return; }
    }
    for (uint32_t j = 0; j < ts; j++) d[j] = cbg_byte<KIND>(F, look, work, p + j);
}
// The point gather: one launch per kind that occurs among the jobs of points; gjob / gblk / rows are those jobs in launch order.  A thread has
// one point of its job (cbp_thread), 256 points to a workgroup.  KIND reaches cbp_item alone, where the two bit-shuffle kinds have the plain
// body only: jobs of kind CBG_BITUN4 run the CBG_BITUN instantiation under their own stage name (cbr_items_kind).
template <int KIND>
__global__ __launch_bounds__(256) void k_cbp_gather(const CbgFrame *__restrict__ frames, const CbxJob *__restrict__ jobs, const CbpRow *__restrict__ rows,
                                                     const CbgBlock *__restrict__ blocks, const CbPlan *__restrict__ plans, const CbxTouch *__restrict__ touch,
                                                     const CbpPoint *__restrict__ pts, const uint32_t *__restrict__ gjob, const uint32_t *__restrict__ gblk, uint32_t nkind,
                                                     const uint8_t *__restrict__ work) {
    const CbxWg W = cbx_enter(frames, jobs, blocks, plans, touch, gjob, gblk, nkind);
    if (!W.live) return;
    const CbpRow R = rows[W.i];
    uint32_t p;
    if (!cbp_thread(R, W.wl, threadIdx.x, p)) return;
    const CbpPoint P = pts[R.pt0 + p];
    cbp_item<KIND>(W.F, W.look, work, P.off, W.J.dst + P.out);
}
__global__ __launch_bounds__(64) void k_cbx_finish(const CbxJob *__restrict__ jobs, const CbPlan *__restrict__ plans, const CbxTouch *__restrict__ touch, hb_result *results,
                                                    uint32_t njobs) {
    cb_finish_jobs(jobs, plans, results, njobs, &CbxJob::ntl, [touch](const CbxJob &J, uint32_t k) { return touch[J.tl0 + k].rec; });
}

// =====================================================================================================================
// Writing the format.  A stream has to be ONE LZ4 block, and this library's encoder makes blocks of 4 KiB chunks that are
// stitched afterwards -- so the frame is laid out such that nothing needs stitching: blocksize = 4096 x typesize when the
// block is split (typesize <= 16 and a filter is on), else 4096 with the not-split flag; then every stream is exactly one
// matcher chunk, encoded as a block of its own (match_chunk MODE 2).  The filters run per block first (k_cb_shuffle /
// k_cb_bitshuffle, the mirrors of the kernels above), a stream that does not shrink is stored (cbytes == its size, like
// blosc_c), the last, shorter block is one stored stream.  Ratio = the chunk-local encoder's + 4 bytes per stream.
// =====================================================================================================================
// (CbEncPlan: hb_cblosc_enc_batch.h.  The filters' bodies with their workgroup index `bx` and grid size `gx`, as above: k_cbeb_filter passes
// the workgroup's place among those of its frame)
__device__ __forceinline__ void cb_shuffle(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nbytes, uint32_t blocksize, uint32_t ts, uint32_t bx, uint32_t gx) {
    const uint32_t nblocks = (nbytes + blocksize - 1) / blocksize;
    const uint32_t per = blocksize / ts + 1u;
    for (uint64_t i = (uint64_t)bx * blockDim.x + threadIdx.x; i < (uint64_t)nblocks * per; i += (uint64_t)gx * blockDim.x) {
        const uint32_t b = (uint32_t)(i / per), e = (uint32_t)(i % per);
        const uint32_t base = b * blocksize, bsize = nbytes - base < blocksize ? nbytes - base : blocksize, nel = bsize / ts;
        if (e < nel) {
            const uint8_t *s = src + base + (size_t)e * ts;
            uint8_t *d = dst + base + e;
            for (uint32_t j = 0; j < ts; j++) d[(size_t)j * nel] = s[j];
        } else if (e == nel) {
            for (uint32_t k = nel * ts; k < bsize; k++) dst[base + k] = src[base + k];
        }
    }
}
__global__ void k_cb_shuffle(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nbytes, uint32_t blocksize, uint32_t ts) {
    cb_shuffle(dst, src, nbytes, blocksize, ts, blockIdx.x, gridDim.x);
}
__device__ __forceinline__ void cb_bitshuffle(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nbytes, uint32_t blocksize, uint32_t ts, uint32_t bx, uint32_t gx) {
    const uint32_t nblocks = (nbytes + blocksize - 1) / blocksize;
    const uint32_t per = blocksize / (8u * ts) + 1u;
    for (uint64_t i = (uint64_t)bx * blockDim.x + threadIdx.x; i < (uint64_t)nblocks * per; i += (uint64_t)gx * blockDim.x) {
        const uint32_t b = (uint32_t)(i / per), g = (uint32_t)(i % per);
        const uint32_t base = b * blocksize, bsize = nbytes - base < blocksize ? nbytes - base : blocksize, nel = bsize / ts;
        if (nel % 8u != 0u) { for (uint32_t k = g; k < bsize; k += per) dst[base + k] = src[base + k]; continue; }
        const uint32_t ng = nel / 8u;
        if (g < ng) {
            for (uint32_t j = 0; j < ts; j++) {
                uint64_t x = 0;                                                         // byte e = byte j of element 8 g + e
                for (uint32_t e = 0; e < 8u; e++) x |= (uint64_t)src[base + (size_t)(8u * g + e) * ts + j] << (8u * e);
                uint64_t t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull; x ^= t ^ (t << 7);
                t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
                t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
                for (uint32_t k = 0; k < 8u; k++) dst[base + (size_t)(8u * j + k) * ng + g] = (uint8_t)(x >> (8u * k));
            }
        } else if (g == ng) {
            for (uint32_t k = nel * ts; k < bsize; k++) dst[base + k] = src[base + k];
        }
    }
}
__global__ void k_cb_bitshuffle(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nbytes, uint32_t blocksize, uint32_t ts) {
    cb_bitshuffle(dst, src, nbytes, blocksize, ts, blockIdx.x, gridDim.x);
}

struct CbChunkDesc { uint32_t lead, enc_len, last_end, mcode0; };       // = ChunkDesc of hb_lz4_enc.hip
// bytes of stream c in the frame: 4 + the block, or 4 + the chunk itself when the block is no smaller
__device__ __forceinline__ uint32_t cb_stream_bytes(const CbChunkDesc &d) { return 4u + (d.enc_len < HB_CHUNK ? d.enc_len : HB_CHUNK); }
// exclusive prefix sum of the stream sizes, 1024 chunks per tile: tile sums, one workgroup over the tiles, offsets
// (fused_nblk != 0: the descriptors / records come from the fused shuffle + match kernel, stream (block b, plane j) at index j * nblk + b)
__device__ __forceinline__ uint32_t cb_desc_index(uint32_t c, uint32_t nsplit, uint32_t fused_nblk) { return fused_nblk ? (c % nsplit) * fused_nblk + c / nsplit : c; }
// (bodies with the tile index `bx` among the frame's tiles and their LDS handed in: the one-frame kernels pass blockIdx.x, the batch kernels
// k_cbeb_* the tile's place in its frame and that frame's descriptors, tile sums and plan)
__device__ __forceinline__ void cbe_tiles(const CbChunkDesc *__restrict__ desc, uint32_t nchunks, uint32_t nsplit, uint32_t fused_nblk, uint32_t *__restrict__ tile_sum, uint32_t bx,
                                          uint32_t *s) {
    const uint32_t t0 = bx * 1024u;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < 4u; k++) { const uint32_t c = t0 + k * 256u + threadIdx.x; if (c < nchunks) sum += cb_stream_bytes(desc[cb_desc_index(c, nsplit, fused_nblk)]); }
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0) tile_sum[bx] = s[0];
}
__global__ __launch_bounds__(256) void k_cbe_tiles(const CbChunkDesc *__restrict__ desc, uint32_t nchunks, uint32_t nsplit, uint32_t fused_nblk, uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t s[256];
    cbe_tiles(desc, nchunks, nsplit, fused_nblk, tile_sum, blockIdx.x, s);
}
__device__ __forceinline__ void cbe_scan(uint32_t *tile_sum, uint32_t ntiles, CbEncPlan *plan, uint32_t *s) {
    const int t = threadIdx.x;
    // (ntiles <= 1024: inputs below 4 GiB)
    const uint32_t v = (uint32_t)t < ntiles ? tile_sum[t] : 0u;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { const uint32_t y = t >= d ? s[t - d] : 0u; __syncthreads(); s[t] += y; __syncthreads(); }
    if ((uint32_t)t < ntiles) tile_sum[t] = s[t] - v;
    if (t == 1023) plan->total = s[1023];
}
__global__ __launch_bounds__(1024) void k_cbe_scan(uint32_t *tile_sum, uint32_t ntiles, CbEncPlan *plan) {
    __shared__ uint32_t s[1024];
    cbe_scan(tile_sum, ntiles, plan, s);
}
// plane j of one element block of the fused route (HB_CHUNK elements of nsplit = typesize = 2 / 4 / 8 bytes at e, 16-byte aligned: the fused
// route asks for it) to dst: the chunk that route never materialised.  One wavefront; k_cbe_pack stores it into the frame, k_cbe_zstd into LDS.
__device__ __forceinline__ void cbe_gather_plane(uint8_t *dst, const uint8_t *__restrict__ e, uint32_t j, uint32_t nsplit, int lane) {
    const uint32_t per = 16u / nsplit;                                                     // elements per 16 bytes
    const uint32_t nv = HB_CHUNK * nsplit / 16u;                                           // 512 / 1024 / 2048 vectors: 8 / 16 / 32 per lane
    for (uint32_t i0 = lane; i0 < nv; i0 += 64u * 8u) {                                    // 8 loads in flight per lane
        u32x4 v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = *(const u32x4 *)(e + 16u * (size_t)(i0 + 64u * q));
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t i = i0 + 64u * q;
            const uint32_t wv[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
            uint64_t o = 0;
            for (uint32_t kk = 0; kk < per; kk++) { const uint32_t byte = kk * nsplit + j; o |= (uint64_t)((wv[byte >> 2] >> (8u * (byte & 3u))) & 255u) << (8u * kk); }
            uint8_t *dp = dst + i * per;
            if (per == 8u) st8u(dp, o); else if (per == 4u) st4u(dp, (uint32_t)o); else { dp[0] = (uint8_t)o; dp[1] = (uint8_t)(o >> 8); }
        }
    }
}
// one wavefront per chunk writes { cbytes, block or chunk }; the first chunk of a block also writes the block's bstarts entry.
// 1024 chunks per workgroup of 16 wavefronts: latency-bound small copies, so as many of them in flight as the chip takes.
__device__ __forceinline__ void cbe_pack(const CbChunkDesc *__restrict__ desc, const uint8_t *__restrict__ records, const uint8_t *__restrict__ filtered,
                                         const uint32_t *__restrict__ tile_off, uint32_t nchunks, uint32_t nsplit, uint32_t fused_nblk, uint32_t data0, uint8_t *__restrict__ frame,
                                         uint32_t bx, uint32_t *s, uint32_t *s_off) {
    const uint32_t t0 = bx * 1024u;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t c_mine = t0 + (uint32_t)t;
    const uint32_t mine = c_mine < nchunks ? cb_stream_bytes(desc[cb_desc_index(c_mine, nsplit, fused_nblk)]) : 0u;
    s[t] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { const uint32_t y = t >= d ? s[t - d] : 0u; __syncthreads(); s[t] += y; __syncthreads(); }
    s_off[t] = data0 + tile_off[bx] + s[t] - mine;
    __syncthreads();
    for (uint32_t k = w; k < 1024u; k += 16u) {
        const uint32_t c = t0 + k;
        if (c >= nchunks) break;
        const uint32_t ci = cb_desc_index(c, nsplit, fused_nblk);
        const CbChunkDesc d = desc[ci];
        const uint32_t at = s_off[k];
        const bool stored = d.enc_len >= HB_CHUNK;
        const uint32_t cb = stored ? HB_CHUNK : d.enc_len;
        if (lane < 4) frame[at + lane] = (uint8_t)(cb >> (8 * lane));
        if (lane == 0 && c % nsplit == 0u) { const uint32_t b = c / nsplit; for (int q = 0; q < 4; q++) frame[16u + 4u * b + q] = (uint8_t)(at >> (8 * q)); }
        if (stored && fused_nblk)                                      // no filtered buffer: plane j of element block b, gathered from the input
            cbe_gather_plane(frame + at + 4u, filtered + (size_t)(c / nsplit) * HB_CHUNK * nsplit, c % nsplit, nsplit, lane);
        else wave_copy_g2g(frame + at + 4u, stored ? filtered + (size_t)c * HB_CHUNK : records + (size_t)ci * HB_RSTRIDE, cb, lane);
    }
}
__global__ __launch_bounds__(1024) void k_cbe_pack(const CbChunkDesc *__restrict__ desc, const uint8_t *__restrict__ records, const uint8_t *__restrict__ filtered,
                                                   const uint32_t *__restrict__ tile_off, uint32_t nchunks, uint32_t nsplit, uint32_t fused_nblk, uint32_t data0, uint8_t *__restrict__ frame) {
    __shared__ uint32_t s[1024];
    __shared__ uint32_t s_off[1024];
    cbe_pack(desc, records, filtered, tile_off, nchunks, nsplit, fused_nblk, data0, frame, blockIdx.x, s, s_off);
}
// header, the last (shorter) block as one stored stream (its filtered bytes at `last`), the result
__device__ __forceinline__ void cbe_finish(const CbEncPlan *plan, const uint8_t *__restrict__ last, uint32_t nbytes, uint32_t blocksize, uint32_t ts, uint32_t flags,
                                           uint32_t nfull_blocks, uint32_t data0, uint8_t *__restrict__ frame, uint64_t cap, hb_result *result, int lane) {
    const uint32_t leftover = nbytes - nfull_blocks * blocksize;
    const uint32_t at = data0 + plan->total;
    const uint64_t cbytes = (uint64_t)at + (leftover ? 4u + leftover : 0u);
    if (cbytes > cap || cbytes > 0xFFFFFFFFull) { if (lane == 0) { result->status = HB_ERR_SHORT_BUFFER; result->bytes = 0; result->total_bytes = 0; result->flags = 0; result->reserved = 0; } return; }
    if (leftover) {
        if (lane < 4) { frame[at + lane] = (uint8_t)(leftover >> (8 * lane)); frame[16u + 4u * nfull_blocks + lane] = (uint8_t)(at >> (8 * lane)); }
        wave_copy_g2g(frame + at + 4u, last, leftover, lane);
    }
    if (lane == 0) {
        frame[0] = 2; frame[1] = 1; frame[2] = (uint8_t)flags; frame[3] = (uint8_t)ts;                  // BLOSC_VERSION_FORMAT, LZ4 version format
        for (int q = 0; q < 4; q++) { frame[4 + q] = (uint8_t)(nbytes >> (8 * q)); frame[8 + q] = (uint8_t)(blocksize >> (8 * q)); frame[12 + q] = (uint8_t)((uint32_t)cbytes >> (8 * q)); }
        result->status = HB_OK; result->bytes = cbytes; result->total_bytes = cbytes; result->flags = 0; result->reserved = 0;
    }
}

__global__ __launch_bounds__(64) void k_cbe_finish(const CbEncPlan *plan, const uint8_t *__restrict__ filtered, uint32_t nbytes, uint32_t blocksize, uint32_t ts, uint32_t flags,
                                                   uint32_t nfull_blocks, uint32_t data0, uint8_t *__restrict__ frame, uint64_t cap, hb_result *result) {
    cbe_finish(plan, filtered + (size_t)nfull_blocks * blocksize, nbytes, blocksize, ts, flags, nfull_blocks, data0, frame, cap, result, (int)threadIdx.x);
}

// inputs below one chunk: a memcpyed frame (what c-blosc itself writes for buffers it cannot shrink)
__device__ __forceinline__ void cbe_memcpy_header(uint8_t *frame, uint32_t nbytes, uint32_t ts, uint32_t flags, hb_result *result) {
    const uint32_t cbytes = 16u + nbytes;
    uint32_t bs = nbytes - nbytes % ts; if (bs == 0u) bs = nbytes ? 1u : 0u;
    if (bs > (1u << 29)) bs = (1u << 29) - (1u << 29) % ts;               // (level 0 writes this frame at any size: c-blosc refuses a blocksize above (INT_MAX - 16) / 3)
    frame[0] = 2; frame[1] = 1; frame[2] = (uint8_t)flags; frame[3] = (uint8_t)ts;
    for (int q = 0; q < 4; q++) { frame[4 + q] = (uint8_t)(nbytes >> (8 * q)); frame[8 + q] = (uint8_t)(bs >> (8 * q)); frame[12 + q] = (uint8_t)(cbytes >> (8 * q)); }
    result->status = HB_OK; result->bytes = cbytes; result->total_bytes = cbytes; result->flags = 0; result->reserved = 0;
}
__global__ void k_cbe_memcpy_header(uint8_t *frame, uint32_t nbytes, uint32_t ts, uint32_t flags, hb_result *result) { cbe_memcpy_header(frame, nbytes, ts, flags, result); }

// ---- batches (hb_cblosc_compress_frames_batch_device): many frames through ONE set of launches; the records, prefixes and routes are
// hb_cblosc_enc_batch.h's.  Chunks, tiles and blocks are as independent across frames as inside one, so the bodies above run over flat spaces. ----
// one workgroup per frame: whose every chunk of the map is (gap chunks: nobody's)
__global__ __launch_bounds__(64) void k_cbeb_map(const CbeFrame *__restrict__ frames, uint32_t *__restrict__ chunk_frame) {
    const CbeFrame &F = frames[blockIdx.x];
    for (uint32_t c = threadIdx.x; c < F.mspan; c += 64u) chunk_frame[F.mchunk0 + c] = c < F.nchunks ? blockIdx.x : 0xFFFFFFFFu;
}
// the filter over the flat workgroup space: a frame's first fmain workgroups take its whole blocks (only a frame that is not fused has any),
// the other ftail its last, shorter block
template <bool BITS>
__global__ __launch_bounds__(256) void k_cbeb_filter(const CbeFrame *__restrict__ frames, const uint32_t *__restrict__ fblk, uint32_t nframes, uint8_t *work) {
    const uint32_t k = hb_owner(fblk, nframes, blockIdx.x);
    const CbeFrame &F = frames[k];
    uint32_t bx = blockIdx.x - fblk[k];
    const uint32_t done = F.nfull * F.blocksize;
    if (bx < F.fmain) {
        uint8_t *dst = work + F.fsrc_off;
        if constexpr (BITS) {
            if (F.ffast) cb_bitshuffle4_fast(dst, F.src, F.nfull, F.blocksize, bx, F.fmain);
            else cb_bitshuffle(dst, F.src, done, F.blocksize, F.typesize, bx, F.fmain);
        } else cb_shuffle(dst, F.src, done, F.blocksize, F.typesize, bx, F.fmain);
    } else {
        bx -= F.fmain;
        if constexpr (BITS) cb_bitshuffle(work + F.tail_off, F.src + done, F.nbytes - done, F.blocksize, F.typesize, bx, F.ftail);
        else cb_shuffle(work + F.tail_off, F.src + done, F.nbytes - done, F.blocksize, F.typesize, bx, F.ftail);
    }
}
// one workgroup per tile of the flat tile space (tiles never span two frames)
__global__ __launch_bounds__(256) void k_cbeb_tiles(const CbeFrame *__restrict__ frames, const uint32_t *__restrict__ tile0, uint32_t nframes,
                                                    const CbChunkDesc *__restrict__ desc, uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t s[256];
    const uint32_t k = hb_owner(tile0, nframes, blockIdx.x);
    const CbeFrame &F = frames[k];
    cbe_tiles(desc + F.desc0, F.nchunks, F.nsplit, F.mode == CBE_FUSED ? F.nfull : 0u, tile_sum + F.tile0, blockIdx.x - F.tile0, s);
}
// one workgroup per frame over its tiles (at most 1024 of them: inputs below 2 GiB)
__global__ __launch_bounds__(1024) void k_cbeb_scan(const CbeFrame *__restrict__ frames, uint32_t *tile_sum, CbEncPlan *plans) {
    __shared__ uint32_t s[1024];
    const CbeFrame &F = frames[blockIdx.x];
    if (F.ntiles == 0u) return;                                            // (refused, memcpyed: the plan stays cleared)
    cbe_scan(tile_sum + F.tile0, F.ntiles, plans + blockIdx.x, s);
}
__global__ __launch_bounds__(1024) void k_cbeb_pack(const CbeFrame *__restrict__ frames, const uint32_t *__restrict__ tile0, uint32_t nframes,
                                                    const CbChunkDesc *__restrict__ desc, const uint8_t *__restrict__ records, const uint32_t *__restrict__ tile_off,
                                                    const uint8_t *work) {
    __shared__ uint32_t s[1024];
    __shared__ uint32_t s_off[1024];
    const uint32_t k = hb_owner(tile0, nframes, blockIdx.x);
    const CbeFrame &F = frames[k];
    const bool fused = F.mode == CBE_FUSED;
    const uint8_t *filtered = F.fsrc_off ? work + F.fsrc_off : F.src;      // (fused: the input itself, the stored planes are gathered from it)
    cbe_pack(desc + F.desc0, records + (size_t)F.desc0 * HB_RSTRIDE, filtered, tile_off + F.tile0, F.nchunks, F.nsplit, fused ? F.nfull : 0u, 16u + 4u * F.nblocks, F.dst,
             blockIdx.x - F.tile0, s, s_off);
}
// one wavefront per frame: what the host decided, the memcpyed frame, or k_cbe_finish's header, last block and record
__global__ __launch_bounds__(64) void k_cbeb_finish(const CbeFrame *__restrict__ frames, const CbEncPlan *plans, const uint8_t *work, hb_result *results) {
    const uint32_t k = blockIdx.x;
    const int lane = threadIdx.x;
    const CbeFrame &F = frames[k];
    hb_result *r = results + k;
    if (F.mode == CBE_REFUSED) {
        if (lane == 0) { r->status = F.status; r->flags = 0; r->bytes = 0; r->total_bytes = 0; r->reserved = 0; }
        return;
    }
    if (F.mode == CBE_MEMCPY) {
        wave_copy_g2g(F.dst + 16, F.src, F.nbytes, lane);
        if (lane == 0) cbe_memcpy_header(F.dst, F.nbytes, F.typesize, F.flags, r);
        return;
    }
    const uint8_t *last = F.tail_off ? work + F.tail_off : F.src + (size_t)F.nfull * F.blocksize;
    cbe_finish(plans + k, last, F.nbytes, F.blocksize, F.typesize, F.flags, F.nfull, 16u + 4u * F.nblocks, F.dst, F.cap, r, lane);
}

// ---- writing zstd streams (hb_cblosc_set_stream_format).  The format, the choices and the serial statement are hb_zstd_enc.h's; this is the
// same computation with one wavefront per chunk, between the matcher and the tile sums: the chunk's record (a self-contained LZ4 block) or,
// for a chunk the matcher could not shrink, its plain bytes become one zstd frame, written back over the record slot with enc_len set; a frame
// of HB_CHUNK bytes or more is not written and enc_len = HB_CHUNK marks the chunk stored, so tiles, scan, pack and finish stay as they are.
// Parallel: the record / plane load, the literal copy, the length codes, the histogram (LDS atomics), the (count, value) order, the code
// length sums (a wave scan per Huffman stream, literals dealt out in contiguous slices) and the Huffman bit images (atomicOr into the zeroed
// image: literal i of a stream of T bits lies at [T - incl(i), T - excl(i))).  One lane: the LZ4 parse, the tree, its description, the
// headers and the FSE chain of the sequences.
// frames != NULL: the batch -- workgroup x is chunk x % 1024 of tile x / 1024 of the flat tile space, its frame's descriptors, records, route
// and stored-chunk source (work + fsrc_off, or the frame's input) are the frame record's, as k_cbeb_pack takes them. ----
struct alignas(16) CbeZstdLds {
    ZsEncState S;
    alignas(16) uint32_t img[HB_CHUNK / 4u + 8u];                         // the record on its way in, the zstd frame on its way out
};
__global__ __launch_bounds__(64) void k_cbe_zstd(const CbeFrame *__restrict__ frames, const uint32_t *__restrict__ tile0, uint32_t nframes, CbChunkDesc *desc, uint8_t *records,
                                                 const uint8_t *filtered, uint32_t nchunks, uint32_t nsplit, uint32_t fused_nblk) {
    __shared__ CbeZstdLds Z;
    const int lane = threadIdx.x;
    uint32_t c = blockIdx.x;
    if (frames) {
        const uint32_t tile = blockIdx.x >> 10;
        const CbeFrame &F = frames[hb_owner(tile0, nframes, tile)];
        c = (tile - F.tile0) * 1024u + (blockIdx.x & 1023u);
        nchunks = F.nchunks; nsplit = F.nsplit; fused_nblk = F.mode == CBE_FUSED ? F.nfull : 0u;
        desc += F.desc0; records += (size_t)F.desc0 * HB_RSTRIDE;
        filtered = F.fsrc_off ? filtered + F.fsrc_off : F.src;
    }
    if (c >= nchunks) return;
    ZsEncState *S = &Z.S;
    uint8_t *out = (uint8_t *)Z.img;
    const uint32_t ci = cb_desc_index(c, nsplit, fused_nblk);
    CbChunkDesc *dsc = desc + ci;
    uint8_t *rec = records + (size_t)ci * HB_RSTRIDE;                     // (16-byte aligned: the records' area is, and HB_RSTRIDE is a multiple)
    const uint32_t enc_len = dsc->enc_len;
    const bool stored = enc_len >= HB_CHUNK;
    if (!stored) {                                                        // (the vectors end inside the slot: enc_len < HB_CHUNK < HB_RSTRIDE)
        for (uint32_t i = lane; i < (enc_len + 15u) / 16u; i += 64u) *(u32x4 *)(out + 16u * i) = *(const u32x4 *)(rec + 16u * i);
        wave_sync();
        if (lane == 0) S->use_huf = zse_parse(S, out, enc_len, HB_CHUNK) ? 1u : 0u;
        wave_sync();
        if (!S->use_huf) { if (lane == 0) dsc->enc_len = HB_CHUNK; return; }      // (not a block of this chunk: the plain bytes go out)
        zse_copy_lits(S, out, (uint32_t)lane, 64u);
        zse_seq_codes(S, (uint32_t)lane, 64u);
    } else {
        if (fused_nblk) cbe_gather_plane(S->lit, filtered + (size_t)(c / nsplit) * HB_CHUNK * nsplit, c % nsplit, nsplit, lane);
        else {
            const uint8_t *p = filtered + (size_t)c * HB_CHUNK;
            for (uint32_t i = lane; i < HB_CHUNK / 16u; i += 64u) *(u32x4 *)(S->lit + 16u * i) = ld16u(p + 16u * i);
        }
        if (lane == 0) zse_plain(S, HB_CHUNK);
    }
    for (uint32_t s = lane; s < 256u; s += 64u) S->cnt[s] = 0u;
    wave_sync();
    const uint32_t nlit = S->nlit;
    for (uint32_t i = lane; i < nlit; i += 64u) atomicAdd(&S->cnt[S->lit[i]], 1u);
    wave_sync();
    if (lane == 0) zse_alphabet(S);
    wave_sync();
    const uint32_t fh = 7u;                                               // the frame header of HB_CHUNK bytes: magic, descriptor, two bytes of size
    uint32_t total = 0u;                                                  // (wave-uniform) the frame's length, 0: the chunk is stored
    if (S->nsym == 1u) {
        if (lane == 0) { zse_frame_header(out, HB_CHUNK, HB_CHUNK); zse_block_header(out, fh, 1u, HB_CHUNK); out[fh + 3u] = S->lit[0]; }
        total = fh + 4u;
    } else {
        zse_rank(S, (uint32_t)lane, 64u);
        wave_sync();
        if (lane == 0) { S->tree_n = 0u; if (zse_lengths(S)) zse_tree(S); zse_lit_split(S); }
        wave_sync();
        const uint32_t nstreams = S->nstreams, have_tree = S->tree_n, seg = S->scnt[0];
        uint32_t pre[4];                                                  // the code bits of stream k in front of my slice (k is unrolled: registers)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t sum = 0u;
            if ((uint32_t)k < nstreams && have_tree) {
                const uint32_t n = S->scnt[k], per = (n + 63u) / 64u, a = min((uint32_t)lane * per, n), e = min(a + per, n);
                const uint8_t *p = S->lit + (uint32_t)k * seg;
                for (uint32_t i = a; i < e; i++) sum += S->len[p[i]];
            }
            const uint32_t incl = wave_incl_scan_dpp(sum);
            pre[k] = incl - sum;
            const uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (lane == 0) S->sbits[k] = bits;
        }
        for (uint32_t i = lane; i < HB_CHUNK / 4u + 8u; i += 64u) Z.img[i] = 0u;
        wave_sync();
        if (lane == 0) { zse_frame_header(out, HB_CHUNK, HB_CHUNK); if (!zse_lit_header(S, out, fh + 3u, HB_CHUNK)) S->lit_end = 0u; }
        wave_sync();
        if (S->lit_end) {
            if (S->use_huf) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if ((uint32_t)k >= nstreams) continue;
                    const uint32_t n = S->scnt[k], per = (n + 63u) / 64u, a = min((uint32_t)lane * per, n), e = min(a + per, n);
                    const uint8_t *p = S->lit + (uint32_t)k * seg;
                    const uint32_t top = 8u * S->sat[k] + S->sbits[k];    // the marker's bit; everything below ends inside the stream's bytes
                    uint32_t pos = top - pre[k];
                    for (uint32_t i = a; i < e; i++) {
                        const uint32_t sym = p[i];
                        pos -= S->len[sym];
                        const uint64_t v = (uint64_t)S->code[sym] << (pos & 31u);
                        atomicOr(&Z.img[pos >> 5], (uint32_t)v);
                        if (v >> 32) atomicOr(&Z.img[(pos >> 5) + 1u], (uint32_t)(v >> 32));
                    }
                    if (lane == 0) atomicOr(&Z.img[top >> 5], 1u << (top & 31u));
                }
            } else for (uint32_t i = lane; i < nlit; i += 64u) out[S->lit_at + i] = S->lit[i];
            wave_sync();
            if (lane == 0) {
                const uint32_t end = zse_sequences(S, out, S->lit_end, HB_CHUNK);
                if (end && end < HB_CHUNK) zse_block_header(out, fh, 2u, end - fh - 3u);
                S->lit_end = end < HB_CHUNK ? end : 0u;
            }
            wave_sync();
            total = S->lit_end;
        }
    }
    wave_sync();
    if (total) {                                                          // (nothing reads the slot any more: the record was taken into LDS first)
        for (uint32_t i = lane; i < (total + 15u) / 16u; i += 64u) *(u32x4 *)(rec + 16u * i) = *(const u32x4 *)(out + 16u * i);
        if (lane == 0) dsc->enc_len = total;
    } else if (!stored && lane == 0) dsc->enc_len = HB_CHUNK;
}

// ---- batched box writes (hb_cblosc_compress_boxes_batch_device; the host side and the index arithmetic are hb_cblosc_enc_box_batch.h): the
// chunks that are not read where they lie are assembled in the workspace, then the batch above runs over them. ----
struct CbxeDeviceIO {
    __device__ __forceinline__ void copy16(uint8_t *d, const uint8_t *s) { *(u32x4 *)d = ld16u_nt(s); }      // (the source is read once; the staged chunk is read next)
    __device__ __forceinline__ void fill16(uint8_t *d, const uint8_t *s) { *(u32x4 *)d = ld16u(s); }
    __device__ __forceinline__ void put(uint8_t *d, uint8_t v) { *d = v; }
    __device__ __forceinline__ uint8_t get(const uint8_t *s) { return *s; }
};
// One launch over the workgroup prefix of the staged jobs.  A thread owns one 16-byte unit of its job's staged chunk (cbxe_thread): one
// unaligned 16-byte load and one aligned store inside the box, one aligned store of the rotated fill pattern outside, byte by byte where the
// unit crosses the box's edge or a chunk row.  The source is read only at the box's items.
__global__ __launch_bounds__(256) void k_cbxe_gather(const CbxeJob *__restrict__ jobs, const uint32_t *__restrict__ gblk, uint32_t njobs, const uint8_t *__restrict__ table,
                                                      uint32_t ts, uint64_t rcp_ts) {
    const uint32_t i = hb_owner(gblk, njobs, blockIdx.x);
    CbxeDeviceIO io;
    cbxe_thread(jobs[i], table, ts, rcp_ts, blockIdx.x - gblk[i], threadIdx.x, io);
}

// ---- batched box updates (hb_cblosc_update_boxes_batch_device; the host side and the index arithmetic are hb_cblosc_upd_box_batch.h): the
// staged chunk holds the base already (the gather's fill, or the batch decoder's bytes); the overlay puts the box's items over it. ----
struct CbxuDeviceIO {
    __device__ __forceinline__ void copy16(uint8_t *d, const uint8_t *s) { *(u32x4 *)d = ld16u_nt(s); }      // (the source is read once; the staged chunk is read next)
    __device__ __forceinline__ void put(uint8_t *d, uint8_t v) { *d = v; }
    __device__ __forceinline__ uint8_t get(const uint8_t *s) { return *s; }
};
// One launch over the workgroup prefix of the overlay jobs.  A thread owns one 16-byte-aligned slice of the staged chunk intersected with one
// box row (cbxu_thread): one unaligned non-temporal 16-byte load and one aligned 16-byte store where the slice is whole, byte by byte where
// the row's ends clip it.  Work is proportional to the box; no byte outside the box is stored, no source byte outside its items is read.
__global__ __launch_bounds__(256) void k_cbxu_overlay(const CbxuJob *__restrict__ jobs, const uint32_t *__restrict__ oblk, uint32_t njobs) {
    const uint32_t i = hb_owner(oblk, njobs, blockIdx.x);
    CbxuDeviceIO io;
    cbxu_thread(jobs[i], blockIdx.x - oblk[i], threadIdx.x, io);
}
// one lane per old-frame job: a base that did not decode spoils its own frame's record, whatever the encoder made of the staged bytes
__global__ __launch_bounds__(64) void k_cbxu_finish(const uint32_t *__restrict__ fin, const hb_result *__restrict__ dres, hb_result *results, uint32_t ndec) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= ndec) return;
    const int32_t st = dres[i].status;
    if (st == 0) return;
    hb_result *r = results + fin[i];
    r->status = st; r->flags = 0; r->bytes = 0; r->total_bytes = 0; r->reserved = 0;
}

// ---- batched selection updates (hb_cblosc_update_index_batch_device; the host side and the index arithmetic are hb_cblosc_upd_index_batch.h): the
// box updates' launch set with two scatters in the overlay's place, the inverse of the index gathers.  The staged chunk holds the base already.
// An index occurs once in a list (the host refuses a repeat), so every chunk byte is stored by at most one thread of at most one of the two
// launches: the new frame does not depend on the order the threads run in. ----
template <class T> struct __attribute__((packed, aligned(1))) hb_unaligned { T v; };
struct CbiuDeviceIO {
    typedef u32x4 V16;
    __device__ __forceinline__ void copy16(uint8_t *d, const uint8_t *s) { *(u32x4 *)d = ld16u_nt(s); }      // (the source is read once; the staged chunk is read next)
    __device__ __forceinline__ void put(uint8_t *d, uint8_t v) { *d = v; }
    __device__ __forceinline__ uint8_t get(const uint8_t *s) { return *s; }
    __device__ __forceinline__ V16 load16(const uint8_t *s) { return ld16u_nt(s); }
    // a point table entry (16-byte aligned), whole
    __device__ __forceinline__ CbpPoint point(const CbpPoint *p) { const u32x4 v = *(const u32x4 *)p; return CbpPoint{v.x, v.y, (uint64_t)v.z | ((uint64_t)v.w << 32)}; }
    // item c of v (c is a constant once the caller's loop is unrolled), TS bytes, to a destination aligned to TS
    template <uint32_t TS>
    __device__ __forceinline__ void item(uint8_t *d, const V16 &v, uint32_t c) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if constexpr (TS == 1u) *d = (uint8_t)(w[c >> 2] >> (8u * (c & 3u)));
        else if constexpr (TS == 2u) *(uint16_t *)d = (uint16_t)(w[c >> 1] >> (16u * (c & 1u)));
        else if constexpr (TS == 4u) *(uint32_t *)d = w[c];
        else if constexpr (TS == 8u) *(uint64_t *)d = (uint64_t)w[2u * c] | ((uint64_t)w[2u * c + 1u] << 32);
        else *(u32x4 *)d = v;
    }
    template <uint32_t TS>
    __device__ __forceinline__ void copy_item(uint8_t *d, const uint8_t *s) {
        if constexpr (TS == 1u) *d = *s;
        else if constexpr (TS == 2u) *(uint16_t *)d = ((const hb_unaligned<uint16_t> *)s)->v;
        else if constexpr (TS == 4u) *(uint32_t *)d = ((const hb_unaligned<uint32_t> *)s)->v;
        else if constexpr (TS == 8u) *(uint64_t *)d = ((const hb_unaligned<uint64_t> *)s)->v;
        else *(u32x4 *)d = ld16u(s);
    }
};
// The rows scatter: the row is a plain run.  One launch over the workgroup prefix of its jobs.  A thread owns one 16-byte-aligned slice of the
// staged chunk intersected with one selected row (cbiu_thread_rows): one unaligned non-temporal 16-byte load and one aligned 16-byte store
// where the slice is whole, byte by byte where the row's ends clip it; only the row's chunk offset and source offset come from tables or steps.
__global__ __launch_bounds__(256) void k_cbiu_scatter_rows(const CbiuJob *__restrict__ jobs, const uint32_t *__restrict__ blk, uint32_t njobs, const CbiuPair *__restrict__ tab) {
    const uint32_t i = hb_owner(blk, njobs, blockIdx.x);
    CbiuDeviceIO io;
    cbiu_thread_rows(jobs[i], tab, blockIdx.x - blk[i], threadIdx.x, io);
}
// The items scatter: the row is stepped or listed.  A thread owns cbs_items_per_unit(ts) consecutive selection items of a row
// (cbiu_thread_items): without a src_list that is 16 contiguous source bytes, loaded once; each item is stored whole by one instruction for
// typesize 1, 2, 4, 8 or 16, byte by byte for the others.  With a src_list the source is read per item.
__global__ __launch_bounds__(256) void k_cbiu_scatter_items(const CbiuJob *__restrict__ jobs, const uint32_t *__restrict__ blk, uint32_t njobs, const CbiuPair *__restrict__ tab,
                                                             uint32_t ts) {
    const uint32_t i = hb_owner(blk, njobs, blockIdx.x);
    CbiuDeviceIO io;
    cbiu_thread_items(jobs[i], tab, ts, blockIdx.x - blk[i], threadIdx.x, io);
}

// ---- batched point updates (hb_cblosc_update_points_batch_device; the host side and the thread are hb_cblosc_upd_point_batch.h): the box
// updates' launch set with one scatter in the overlay's place, the inverse of the point gather.  One launch over the workgroup prefix of the
// jobs that have points.  A thread owns one point (cbpu_thread): one 16-byte table load, coalesced over the workgroup, one item load of any
// alignment from the source, one item store -- a single instruction for typesize 1, 2, 4, 8 and 16, byte by byte for the others.  An item
// occurs once in a job (the host refuses a repeat), so every chunk byte is stored by at most one thread: the new frame does not depend on
// the order the threads run in.  No LDS, no atomics. ----
__global__ __launch_bounds__(256) void k_cbpu_scatter_points(const CbpuJob *__restrict__ jobs, const uint32_t *__restrict__ blk, uint32_t njobs, const CbpPoint *__restrict__ tab,
                                                              uint32_t ts) {
    const uint32_t i = hb_owner(blk, njobs, blockIdx.x);
    CbiuDeviceIO io;
    cbpu_thread(jobs[i], tab, ts, blockIdx.x - blk[i], threadIdx.x, io);
}

// ---- the device builder of a prepared point selection (hb_cblosc_point_sel_create_device; the records, the grouping and the thread are
// hb_cblosc_point_sel.h).  One launch per group of jobs over the workgroup prefix of the group's jobs; a thread owns one point (cbsel_thread):
// one 16-byte load of the caller's point, the checks, one 16-byte store of its table entry, the marks of the one or two blocks the item
// touches in the job's block bitmap, its own bit in the job's item bitmap -- an OR that finds the bit set is a repeat -- and `out + 1` into the
// job's 64-bit maximum.  Atomic traffic stays low: an OR is skipped where a relaxed load shows its bit already (clustered points share block
// bits, and a word once raised stays raised), and the maximum is reduced across the wave before lane 0's single atomic.  Bits are only ever
// set, so a stale load costs an OR and never an answer.  Vector atomics and plain C++; no LDS. ----
struct CbselDeviceIO {
    __device__ __forceinline__ hb_cblosc_point load_point(const hb_cblosc_point *p) {
        const u32x4 v = *(const u32x4 *)p;
        return hb_cblosc_point{(int64_t)((uint64_t)v.x | ((uint64_t)v.y << 32)), (int64_t)((uint64_t)v.z | ((uint64_t)v.w << 32))};
    }
    __device__ __forceinline__ void store_entry(CbpPoint *d, const CbpPoint &e) {
        u32x4 v; v.x = e.off; v.y = 0u; v.z = (uint32_t)e.out; v.w = (uint32_t)(e.out >> 32);
        *(u32x4 *)d = v;
    }
    __device__ __forceinline__ bool mark(uint32_t *words, uint64_t bit) {
        uint32_t *w = words + (bit >> 5);
        const uint32_t m = 1u << ((uint32_t)bit & 31u);
        if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) return true;
        return (atomicOr(w, m) & m) != 0u;
    }
    __device__ __forceinline__ void raise(uint32_t *w) {
        if (!__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(w, 1u);
    }
    // (every lane of the wave is here: cbsel_thread has no early exit, and a workgroup is four whole waves)
    __device__ __forceinline__ void fold_max(uint64_t *w, uint64_t v) {
        for (int d = 32; d; d >>= 1) {
            const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
            v = o > v ? o : v;
        }
        if ((threadIdx.x & 63u) == 0u && v) atomicMax((unsigned long long *)w, (unsigned long long)v);
    }
};
__global__ __launch_bounds__(256) void k_cbsel_build(const CbselJob *__restrict__ jobs, const uint32_t *__restrict__ blk, uint32_t njobs, const hb_cblosc_point *__restrict__ in,
                                                      CbpPoint *__restrict__ tab, uint32_t ts, uint64_t out_lim, uint32_t *ibits, uint32_t *bbits, CbselOut *outs) {
    const uint32_t i = hb_owner(blk, njobs, blockIdx.x);
    CbselDeviceIO io;
    cbsel_thread(jobs[i], in, tab, ts, out_lim, ibits, bbits, outs + i, blockIdx.x - blk[i], threadIdx.x, io);
}

// ---- selections from a device mask or device coordinate arrays of the whole array (hb_cblosc_point_sel_create_mask_device / _coords_device;
// the geometry, the row arithmetic and the bodies of the threads are hb_cblosc_array_sel.h).  Every dependency between workgroups is a kernel
// boundary.  Mask: k_cbas_mask_count (a wave per chunk row: its selected bytes), the two prefix sums over the row counts -- chunk-major and
// array order -- by k_cbas_tiles / k_cbas_scan / k_cbas_apply, k_cbas_chunks ({first, count} per chunk: what comes down), k_cbas_mask_emit (a
// wave per row with a selected byte: ballot, mbcnt rank, one 16-byte store per point).  Coordinates: k_cbas_coord_bucket (a thread per point:
// its slot from its chunk's counter, large groups of a wave on one chunk sharing the atomic add), the prefix sum over the counters,
// k_cbas_coord_place.  No LDS beyond the scans' four words. ----
#define CBAS_MERGE_MIN 8u                // lanes of a wave on one chunk that share an atomic add (take_slot)
struct CbasDeviceIO {
    __device__ __forceinline__ uint32_t load8(const uint8_t *p) { return *p; }
    __device__ __forceinline__ CbasVec load16(const uint8_t *p) { const u32x4 v = *(const u32x4 *)p; return CbasVec{v.x, v.y, v.z, v.w}; }
    __device__ __forceinline__ uint32_t load32(const uint32_t *p) { return *p; }
    __device__ __forceinline__ void store32(uint32_t *p, uint32_t v) { *p = v; }
    __device__ __forceinline__ int64_t load_i64(const int64_t *p) { return *p; }
    __device__ __forceinline__ void store_pair(uint32_t *p, uint32_t a, uint32_t b) { u32x2 v; v.x = a; v.y = b; *(u32x2 *)p = v; }
    __device__ __forceinline__ void store_point(hb_cblosc_point *p, const hb_cblosc_point &pt) {
        u32x4 v; v.x = (uint32_t)pt.item; v.y = (uint32_t)((uint64_t)pt.item >> 32); v.z = (uint32_t)pt.out; v.w = (uint32_t)((uint64_t)pt.out >> 32);
        *(u32x4 *)p = v;
    }
    __device__ __forceinline__ CbasRec load_rec(const CbasRec *p) { const u32x4 v = *(const u32x4 *)p; return CbasRec{v.x, v.y, v.z, v.w}; }
    __device__ __forceinline__ void store_rec(CbasRec *p, const CbasRec &r) { u32x4 v; v.x = r.chunk; v.y = r.slot; v.z = r.item; v.w = r.pad; *(u32x4 *)p = v; }
    // (every lane of the wave is here: the kernel's only exit in front of it is the whole wave's)
    __device__ __forceinline__ void row_sum(uint32_t *p, uint32_t v) {
        for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((threadIdx.x & 63u) == 0u) *p = v;
    }
    __device__ __forceinline__ void raise(uint32_t *w) {
        if (!__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(w, 1u);
    }
    // One atomic add per point serialises where many points fall into one chunk (262144 points of one chunk: 3.0 ms of bucket against 0.14 ms
    // for the same points over 256 chunks).  So, while the first lane that still waits has at least CBAS_MERGE_MIN lanes of its wave with it on
    // the same chunk, that group takes its slots with ONE add: the leader adds the group's size and every member gets the answer plus its
    // rank in the group.  At most 64 / CBAS_MERGE_MIN rounds; whoever is left adds for itself.  (The lanes that are here are the wave's
    // active ones: ballots, the shuffles from the leader and the loop's exits are uniform among them.)
    __device__ __forceinline__ uint32_t take_slot(uint32_t *counters, uint32_t chunk) {
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t slot = 0;
        bool waits = true;
        for (uint32_t round = 0; round < 64u / CBAS_MERGE_MIN; round++) {
            const uint64_t open = __ballot(waits);
            if (!open) break;
            const int leader = __ffsll((unsigned long long)open) - 1;
            const uint32_t c = __shfl(chunk, leader, 64);
            const bool mine = waits && chunk == c;
            const uint64_t peers = __ballot(mine);
            const uint32_t n = (uint32_t)__popcll(peers);
            if (n < CBAS_MERGE_MIN) break;
            uint32_t base = 0;
            if (lane == (uint32_t)leader) base = atomicAdd(counters + c, n);
            base = __shfl(base, leader, 64);
            if (mine) {
                slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
                waits = false;
            }
        }
        if (waits) slot = atomicAdd(counters + chunk, 1u);
        return slot;
    }
};
#define CBAS_ROWS_PER_GROUP 4u           // a wave per chunk row, four waves per workgroup
__global__ __launch_bounds__(256) void k_cbas_mask_count(CbasGeom g, const uint8_t *__restrict__ mask, uint32_t *__restrict__ counts) {
    const uint32_t row = blockIdx.x * CBAS_ROWS_PER_GROUP + (threadIdx.x >> 6);
    if (row >= g.nrows) return;                                           // (the whole wave)
    CbasDeviceIO io;
    cbas_count_thread(g, mask, counts, row, threadIdx.x & 63u, io);
}
__global__ __launch_bounds__(256) void k_cbas_mask_emit(CbasGeom g, const uint8_t *__restrict__ mask, const uint32_t *__restrict__ scan_cm, const uint32_t *__restrict__ scan_ar,
                                                         hb_cblosc_point *__restrict__ pts) {
    const uint32_t row = blockIdx.x * CBAS_ROWS_PER_GROUP + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (row >= g.nrows) return;
    const uint32_t pos = scan_cm[row], n = scan_cm[row + 1u] - pos;
    if (!n) return;                                                       // (most rows of a sparse mask end here)
    CbasDeviceIO io;
    const CbasRow R = cbas_row(g, row);
    const uint32_t out = scan_ar[R.arow];
    // (the row has n selected bytes, so the walk ends inside it; a mask that changed since the count neither walks on nor writes past the row's n entries)
    for (uint32_t step = 0, run = 0; run < n && step * 64u < R.len; step++) {
        const bool pred = cbas_emit_pred(mask, R, step, lane, io);
        const uint64_t ballot = __ballot(pred);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
        cbas_emit_store(pts, R, pos + run, out + run, n - run, step, lane, pred, rank, io);
        run += (uint32_t)__popcll(ballot);
    }
}
// the exclusive prefix of v over the workgroup's 256 threads and its total; s_w: four words of LDS, free again when it returns
__device__ __forceinline__ uint32_t cbas_block_excl(uint32_t v, uint32_t *s_w, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += o;
    }
    if (lane == 63u) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    for (uint32_t k = 0; k < 4u; k++) { const uint32_t x = s_w[k]; base += k < w ? x : 0u; total += x; }
    __syncthreads();
    return base + inc - v;
}
// blockIdx.y: the order (0: as the counts lie; 1: array order, the mask form's second sum); its tile sums and prefixes lie ntiles words further on
__global__ __launch_bounds__(256) void k_cbas_tiles(CbasGeom g, const uint32_t *__restrict__ counts, uint32_t n, uint32_t ntiles, uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t s_w[4];
    CbasDeviceIO io;
    uint32_t total;
    cbas_block_excl(cbas_tile_thread(g, counts, blockIdx.y, n, blockIdx.x, threadIdx.x, io), s_w, total);
    if (threadIdx.x == 0u) tile_sum[(size_t)blockIdx.y * ntiles + blockIdx.x] = total;
}
// one workgroup per order: the exclusive prefix of the tile sums
__global__ __launch_bounds__(256) void k_cbas_scan(const uint32_t *__restrict__ tile_sum, uint32_t *__restrict__ tile_pre, uint32_t ntiles) {
    __shared__ uint32_t s_w[4];
    tile_sum += (size_t)blockIdx.x * ntiles; tile_pre += (size_t)blockIdx.x * ntiles;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += 256u) {                // (uniform: every thread takes every barrier)
        const uint32_t i = base + threadIdx.x;
        uint32_t total;
        const uint32_t excl = cbas_block_excl(i < ntiles ? tile_sum[i] : 0u, s_w, total);
        if (i < ntiles) tile_pre[i] = carry + excl;
        carry += total;
    }
}
__global__ __launch_bounds__(256) void k_cbas_apply(CbasGeom g, const uint32_t *__restrict__ counts, uint32_t n, uint32_t ntiles, const uint32_t *__restrict__ tile_pre,
                                                     uint32_t *__restrict__ out0, uint32_t *__restrict__ out1) {
    __shared__ uint32_t s_w[4];
    CbasDeviceIO io;
    uint32_t total;
    const uint32_t excl = cbas_block_excl(cbas_tile_thread(g, counts, blockIdx.y, n, blockIdx.x, threadIdx.x, io), s_w, total);
    cbas_apply_thread(g, counts, blockIdx.y, n, blockIdx.x, threadIdx.x, tile_pre[(size_t)blockIdx.y * ntiles + blockIdx.x] + excl, blockIdx.y ? out1 : out0, io);
}
__global__ __launch_bounds__(256) void k_cbas_chunks(CbasGeom g, const uint32_t *__restrict__ scan_cm, uint32_t *__restrict__ pairs) {
    CbasDeviceIO io;
    cbas_chunk_thread(g, scan_cm, pairs, blockIdx.x * 256u + threadIdx.x, io);
}
__global__ __launch_bounds__(256) void k_cbas_coord_bucket(CbasGeom g, CbasCoords X, uint32_t npoints, uint32_t *counters, uint32_t *flag, CbasRec *__restrict__ rec) {
    CbasDeviceIO io;
    cbas_bucket_thread(g, X, npoints, blockIdx.x * 256u + threadIdx.x, counters, flag, rec, io);
}
__global__ __launch_bounds__(256) void k_cbas_coord_place(const CbasRec *__restrict__ rec, const uint32_t *__restrict__ first, hb_cblosc_point *__restrict__ pts, uint32_t npoints) {
    CbasDeviceIO io;
    cbas_place_thread(rec, first, pts, npoints, blockIdx.x * 256u + threadIdx.x, io);
}

void hb_launch_match_selfcontained(const uint8_t *src, size_t n, void *desc, uint8_t *records, uint32_t nchunks, int ways, int accel, hipStream_t s);   // hb_lz4_enc.hip
bool hb_launch_match_fused_selfcontained(const uint8_t *src, int typesize, void *desc, uint8_t *records, uint32_t nblk, int ways, int accel, hipStream_t s);
void hb_launch_match_selfcontained_batch(const BatchFrame *bf, const uint32_t *chunk_frame, void *desc, uint8_t *records, uint32_t total_chunks, int ways, int accel, hipStream_t s);
bool hb_launch_match_fused_selfcontained_batch(const BatchFrame *bf, const uint32_t *chunk_frame, int typesize, void *desc, uint8_t *records, uint32_t total_items, int ways,
                                               int accel, hipStream_t s);

struct CbEncLayout { size_t plan, tiles, desc, records, filtered, total; uint32_t blocksize, nsplit, nblocks, nfull, nchunks, ntiles; };
static CbEncLayout cbe_layout(size_t n, int shuffle, int typesize) {
    CbEncLayout L;
    const CbeGeom G = cbe_geom(n, shuffle, typesize);                     // (hb_cblosc_enc_batch.h: one geometry for this call and for the batch)
    L.nsplit = G.nsplit; L.blocksize = G.blocksize; L.nblocks = G.nblocks; L.nfull = G.nfull; L.nchunks = G.nchunks; L.ntiles = G.ntiles;
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += cb_align(b); return at; };
    L.plan = take(sizeof(CbEncPlan));
    L.tiles = take((size_t)(L.ntiles + 1) * 4);
    L.desc = take((size_t)L.nchunks * sizeof(CbChunkDesc));
    L.records = take((size_t)L.nchunks * HB_RSTRIDE + 256);
    L.filtered = take(n + 64);
    L.total = o;
    return L;
}

// launch shape of the 16-byte-per-lane filter kernel (k_cb_bitshuffle4_fast): every thread gets ONE work item, no grid-stride passes (round 3,
// tools/lab/filter_lab.hip: streaming kernels on this chip want the dispatcher to deal out the work: 0.76 -> 0.55 ms).  The byte-gathering
// kernels (k_cb_unshuffle & co.) are the opposite case: the same change took them from 0.61 to 0.88 ms -- they keep their 2048 workgroups.
static inline unsigned cb_grid(uint64_t items) { const uint64_t g = (items + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > (1u << 24) ? (1u << 24) : g)); }

// plan, stream decoders and per-block un-filter for blocks [b0, b0 + nblocks) of the frame: `out` receives their `nbytes` bytes (all of the
// frame for b0 = 0; the last block of the frame may be shorter).  streams: nblocks * nsplit records, staged: nbytes + 64 bytes.
static void cb_launch_blocks(const hb_cblosc_header *hdr, const uint8_t *d_frame, size_t n, uint32_t b0, uint32_t nblocks, uint32_t nbytes, uint8_t *out,
                             CbPlan *plan, CbStream *streams, uint8_t *staged, hipStream_t s) {
    const uint32_t blocksize = hdr->blocksize, ts = hdr->typesize, flags = cb_record_flags(*hdr);      // (the codec as the frame was accepted: k_cb_plan's bound)
    const uint32_t nsplit = cb_nsplit(flags, ts, blocksize);
    // blosc_d: the byte shuffle counts for typesize > 1 only (and comes first), the bit shuffle for any typesize
    const bool unshuf = (flags & CB_FLAG_SHUFFLE) && ts > 1, unbit = !unshuf && (flags & CB_FLAG_BITSHUFFLE);
    const bool filtered = unshuf || unbit;
    uint8_t *target = filtered ? staged : out;
    const uint32_t nstreams = nblocks * nsplit;
    hb_prof_begin("k_cb_plan", s);
    hipLaunchKernelGGL(k_cb_plan, dim3((nblocks + 63) / 64), dim3(64), 0, s, d_frame, (uint64_t)n, hdr->nbytes, blocksize, hdr->cbytes, ts, flags, plan, streams, b0, nblocks);
    hb_prof_end(s);
    const bool blz = hdr->codec_format == CB_CODEC_BLOSCLZ;              // (accepted by the caller: hb_cblosc_accept_codecs)  One codec per frame: its decoder alone
    const bool zstd = hdr->codec_format == CB_CODEC_ZSTD;
    const bool zlib = hdr->codec_format == CB_CODEC_ZLIB;
    const bool small = !blz && !zstd && !zlib && blocksize / nsplit <= HB_CHUNK;           // streams of at most one chunk: the LDS-resident decoder takes them
    if (!blz && !zstd && !zlib && !small) { hb_prof_begin("k_cb_decode_small", s); hb_prof_end(s); }      // (every LZ4 frame reports the same stages, this one empty here: the rate tools' tables key on them)
    cb_launch_streams(CbOneSpace{d_frame, plan, target, (int)hdr->codec_format, small}, streams, nstreams, small, !blz && !zstd && !zlib, blz, zstd, zlib, nsplit, "k_cb_decode_small", "k_cb_decode",
                      "k_cb_decode_blz", "k_cb_decode_zstd", "k_cb_decode_zlib", s);
    if (filtered) {
        hb_prof_begin("k_cb_unfilter", s);
        if (unshuf)
            {
            // whole blocks of whole 1024-element tiles: the tile kernels of hb_filters.hip, block by block (6 TB/s instead of the 3.5 of the
            // byte-gathering kernel); a last, shorter block -- or any other shape -- the plain way
            const uint32_t nfull = nbytes / blocksize, tail = nbytes - nfull * blocksize;
            if (hb_launch_shuffle_blocks(true, out, staged, nfull, blocksize, (int)ts, s)) {
                if (tail) hipLaunchKernelGGL(k_cb_unshuffle, dim3(64), dim3(256), 0, s, out + (size_t)nfull * blocksize, staged + (size_t)nfull * blocksize, tail, blocksize, ts);
            } else hipLaunchKernelGGL(k_cb_unshuffle, dim3(2048), dim3(256), 0, s, out, staged, nbytes, blocksize, ts);
        }
        else if (ts == 4u && blocksize % 512u == 0u && nbytes >= blocksize) {       // whole blocks the fast way, a last shorter one the plain way
            const uint32_t nfull = nbytes / blocksize, tail = nbytes - nfull * blocksize;
            hipLaunchKernelGGL(k_cb_bitshuffle4_fast<false>, dim3(cb_grid((uint64_t)nfull * (blocksize / 128u))), dim3(256), 0, s, out, staged, nfull, blocksize);
            if (tail) hipLaunchKernelGGL(k_cb_bitunshuffle, dim3(64), dim3(256), 0, s, out + (size_t)nfull * blocksize, staged + (size_t)nfull * blocksize, tail, blocksize, ts);
        } else
            hipLaunchKernelGGL(k_cb_bitunshuffle, dim3(2048), dim3(256), 0, s, out, staged, nbytes, blocksize, ts);
        hb_prof_end(s);
    }
}

// which codec formats the entry points below decode (hb_cblosc_batch.h: cb_codec_refused); every entry point reads it once
static std::atomic<unsigned> g_cb_accept{CB_ACCEPT_DEFAULT};
unsigned hb_cblosc_accepted() { return g_cb_accept.load(std::memory_order_relaxed); }

// what the writers below compress with (include/hipblosc.h, hb_cblosc_set_compressor, hb_cblosc_set_stream_format): one word,
// format << 16 | codec << 8 | clevel, the LZ4 stream format kept as 0 and zstd as HB_CB_FORMAT_ZSTD.  Every writer entry
// point reads it once, before anything is sized or launched, and hands it down to its encode site (hb_cblosc_compress_dev, cbe_launch_batch).
// A host form pins the word it read for its thread while it runs (CbPolicyPin, hb_common.h): the device forms and the one-frame calls it
// answers the rest with then read that word, whatever another thread sets meanwhile.
#define CB_POLICY_DEFAULT ((unsigned)HB_LZ4 << 8 | 5u)
static std::atomic<unsigned> g_cb_policy{CB_POLICY_DEFAULT};
static thread_local int t_cb_policy_pin = -1;
unsigned hb_cblosc_policy() { return t_cb_policy_pin >= 0 ? (unsigned)t_cb_policy_pin : g_cb_policy.load(std::memory_order_relaxed); }
CbPolicyPin::CbPolicyPin() : prev(t_cb_policy_pin) { t_cb_policy_pin = (int)hb_cblosc_policy(); }
CbPolicyPin::~CbPolicyPin() { t_cb_policy_pin = prev; }
// the matcher of a policy word: candidates per bucket and skip acceleration (hb_level_policy, the table of the go-blosc-format frames too);
// level 0: no matcher at all, the frame is memcpyed
// zstd: the streams of a frame that goes through the matcher are written as zstd frames (k_cbe_zstd) and the header names that format
struct CbMatcher { bool store; int ways, accel; bool zstd; };
static inline CbMatcher cb_matcher(unsigned policy) {
    CbMatcher m{(policy & 255u) == 0u, 1, 64, false};
    if (!m.store) { hb_level_policy((int)((policy >> 8) & 255u), (int)(policy & 255u), m.ways, m.accel); m.zstd = (policy >> 16) == (unsigned)HB_CB_FORMAT_ZSTD; }
    return m;
}
// the codec bits 5-7 of a written header's flags: c-blosc's format number of the streams
#define CB_FLAGS_LZ4  (1u << 5)
#define CB_FLAGS_ZSTD 0x80u
// the zstd stage of both encode sites, between the matcher and the tile sums.  One frame: `grid` = its chunks, frames == NULL; a batch: `grid` =
// 1024 x its tiles, the frame records say the rest (k_cbe_zstd).  stored_src: where k_cbe_pack / k_cbeb_pack take a stored chunk from.
static void cbe_zstd_stage(const CbeFrame *d_frames, const uint32_t *d_tile0, uint32_t nframes, uint32_t grid, CbChunkDesc *desc, uint8_t *records, const uint8_t *stored_src,
                           uint32_t nchunks, uint32_t nsplit, uint32_t fused_nblk, hipStream_t s) {
    hb_prof_begin("k_cbe_zstd", s);
    hipLaunchKernelGGL(k_cbe_zstd, dim3(grid), dim3(64), 0, s, d_frames, d_tile0, nframes, desc, records, stored_src, nchunks, nsplit, fused_nblk);
    hb_prof_end(s);
}

extern "C" {

int hb_cblosc_set_compressor(int codec, int clevel) {
    if ((codec != HB_LZ4 && codec != HB_LZ4HC) || clevel < 0 || clevel > 9) return HB_ERR_BAD_ARG;
    unsigned old = g_cb_policy.load(std::memory_order_relaxed);           // (the stream format's bits stay)
    while (!g_cb_policy.compare_exchange_weak(old, (old & ~0xFFFFu) | (unsigned)codec << 8 | (unsigned)clevel, std::memory_order_relaxed)) {}
    return (int)(old & 0xFFFFu);
}
int hb_cblosc_get_compressor(int *codec, int *clevel) {
    const unsigned p = g_cb_policy.load(std::memory_order_relaxed);
    if (codec) *codec = (int)((p >> 8) & 255u);
    if (clevel) *clevel = (int)(p & 255u);
    return HB_OK;
}
int hb_cblosc_set_stream_format(int codec_format) {
    if (codec_format != HB_CB_FORMAT_LZ4 && codec_format != HB_CB_FORMAT_ZSTD) return HB_ERR_BAD_ARG;
    const unsigned bits = codec_format == HB_CB_FORMAT_ZSTD ? (unsigned)HB_CB_FORMAT_ZSTD << 16 : 0u;
    unsigned old = g_cb_policy.load(std::memory_order_relaxed);           // (the compressor's bits stay)
    while (!g_cb_policy.compare_exchange_weak(old, (old & 0xFFFFu) | bits, std::memory_order_relaxed)) {}
    return (old >> 16) ? (int)(old >> 16) : HB_CB_FORMAT_LZ4;
}
int hb_cblosc_get_stream_format(void) {
    const unsigned p = g_cb_policy.load(std::memory_order_relaxed);
    return (p >> 16) ? (int)(p >> 16) : HB_CB_FORMAT_LZ4;
}
// the serial statement of k_cbe_zstd (hb_zstd_enc.h, zs_encode_from_lz4), host only: what the tests without a device hold the writer to
size_t hb_cblosc_zstd_stream_from_lz4(const void *lz4, size_t n, size_t usize, void *dst, size_t cap) {
    if (!lz4 || !dst) return 0;
    std::vector<uint8_t> state(sizeof(ZsEncState));
    return zs_encode_from_lz4((const uint8_t *)lz4, n, usize, (uint8_t *)dst, cap, (ZsEncState *)state.data());
}

#ifdef CB_ZLIB_LAB_NO_ADLER
// the mark of a measurement build: no Makefile target defines the macro, the rate tool asks for this symbol before it times such a library and
// refuses one that has it in an ordinary run
extern "C" int hb_cblosc_lab_no_adler(void) { return 1; }
#endif
int hb_cblosc_accept_codecs(unsigned mask) {
    if (!cb_accept_valid(mask)) return HB_ERR_BAD_ARG;
    return (int)g_cb_accept.exchange(mask, std::memory_order_relaxed);
}

// header fields of a C-Blosc-1 frame (host side); HB_OK or the error a malformed header gets
int hb_cblosc_parse_header(const void *frame, size_t n, hb_cblosc_header *out) { return cb_parse_header(frame, n, out); }

size_t hb_cblosc_decompress_workspace(size_t nbytes, size_t blocksize, size_t typesize) { return cb_decompress_workspace(nbytes, blocksize, typesize); }

// d_frame: the frame in device memory (n bytes available), d_dst: hdr.nbytes bytes.  Asynchronous on `stream`; *d_result says how it went.
int hb_cblosc_decompress_dev(const hb_cblosc_header *hdr, const void *d_frame, size_t n, void *d_dst, size_t cap, void *d_work, size_t work_bytes,
                             hb_result *d_result, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (!hdr || !d_frame || (!d_dst && cap) || !d_work || ((uintptr_t)d_work & 255u) || !d_result) return HB_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const unsigned accept = hb_cblosc_accepted();
    const uint32_t nbytes = hdr->nbytes, blocksize = hdr->blocksize, ts = hdr->typesize, flags = hdr->flags;
    // the record may come from a caller that ignored hb_cblosc_parse_header's return value, or built it itself: repeat its checks
    // before anything divides by a field
    if (hdr->version != 2) return HB_ERR_INVALID_VERSION;
    if (ts == 0u || (nbytes && blocksize == 0u)) return HB_ERR_INVALID_HEADER;
    if (hdr->cbytes > n || hdr->cbytes < 16) return HB_ERR_INVALID_DATA;
    if (nbytes > cap) return HB_ERR_SHORT_BUFFER;
    if (work_bytes < hb_cblosc_decompress_workspace(nbytes, blocksize, ts)) return HB_ERR_SHORT_BUFFER;
    uint8_t *w = (uint8_t *)d_work;
    CbPlan *plan = (CbPlan *)w;
    hipLaunchKernelGGL(k_cb_init, dim3(1), dim3(1), 0, s, plan);
    if (nbytes == 0) { hipLaunchKernelGGL(k_cb_result, dim3(1), dim3(1), 0, s, plan, d_result, (uint64_t)0); return HB_OK; }
    if (flags & CB_FLAG_MEMCPY) {                                       // blosc.c: "memcpyed": the raw bytes follow the header
        if ((uint64_t)hdr->cbytes < 16ull + nbytes) return HB_ERR_INVALID_DATA;
        HB_HIP_TRY(hipMemcpyAsync(d_dst, (const uint8_t *)d_frame + 16, nbytes, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_cb_result, dim3(1), dim3(1), 0, s, plan, d_result, (uint64_t)nbytes);
        return HB_OK;
    }
    if (cb_codec_refused(*hdr, accept)) return HB_ERR_INVALID_CODEC;    // lz4 / lz4hc, and blosclz where the caller has asked for it
    const uint32_t nblocks = (uint32_t)(((uint64_t)nbytes + blocksize - 1) / blocksize);
    if (16ull + 4ull * nblocks > hdr->cbytes) return HB_ERR_INVALID_DATA;
    if (blocksize < ts) return HB_ERR_INVALID_DATA;                     // (c-blosc never writes it; a stream would hold less than one element)
    const uint32_t nsplit = cb_nsplit(flags, ts, blocksize);
    CbStream *streams = (CbStream *)(w + 256);
    uint8_t *staged = w + 256 + cb_align((size_t)nblocks * nsplit * sizeof(CbStream));
    cb_launch_blocks(hdr, (const uint8_t *)d_frame, n, 0u, nblocks, nbytes, (uint8_t *)d_dst, plan, streams, staged, s);
    hipLaunchKernelGGL(k_cb_result, dim3(1), dim3(1), 0, s, plan, d_result, (uint64_t)nbytes);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}

// everything of a batched decode behind cbb_prepare: upload, plan, the decoders, the un-filters, finish over the workspace `w` that B was laid
// out for.  hb_cblosc_decompress_frames_batch_device and hb_cblosc_update_boxes_batch_device both end here.
static int cbb_launch_batch(int nframes, const CbbBatch &B, uint8_t *w, hb_result *d_results, hipStream_t s) {
    const CbbLayout &L = B.L;
    const size_t nf = (size_t)nframes;
    // the frame records, the prefixes and the cleared plans go up in one copy (the buffer is read before the call returns, as with hb_batch.hip's)
    std::vector<uint8_t> up(L.upload, 0);
    memcpy(up.data() + L.frames, B.tab.data(), nf * sizeof(CbbFrame));
    memcpy(up.data() + L.pre, B.pre.data(), nf * 16);
    memcpy(up.data() + L.plans, B.plans.data(), nf * sizeof(CbPlan));
    hb_prof_begin("cbb_upload", s);
    HB_HIP_TRY(hipMemcpyAsync(w, up.data(), L.upload, hipMemcpyHostToDevice, s));
    hb_prof_end(s);
    const CbbFrame *d_frames = (const CbbFrame *)(w + L.frames);
    CbPlan *d_plans = (CbPlan *)(w + L.plans);
    const uint32_t *d_blk0 = (const uint32_t *)(w + L.pre), *d_str0 = d_blk0 + nf, *d_ufrm = d_str0 + nf, *d_ublk = d_ufrm + nf;
    CbStream *d_streams = (CbStream *)(w + L.streams);
    if (B.nstreams) {
        const uint32_t nblocks = (uint32_t)B.nblocks, nstreams = (uint32_t)B.nstreams;
        hb_prof_begin("k_cbb_plan", s);
        hipLaunchKernelGGL(k_cbb_plan, dim3((nblocks + 63u) / 64u), dim3(64), 0, s, d_frames, d_plans, d_blk0, (uint32_t)nframes, nblocks, d_streams);
        hb_prof_end(s);
        cb_launch_streams(CbbSpace{d_frames, d_plans, d_str0, (uint32_t)nframes, w}, d_streams, nstreams, B.any_small, B.any_lz4, B.any_blz, B.any_zstd, B.any_zlib, B.nsplit_all,
                          "k_cbb_decode_small", "k_cbb_decode", "k_cbb_decode_blz", "k_cbb_decode_zstd", "k_cbb_decode_zlib", s);
    }
    for (int k = 0; k < CBK_COUNT; k++) {
        const uint32_t k0 = B.kind0[k], nk = B.kind0[k + 1] - k0, blocks = B.kblocks[k];
        if (!nk) continue;
        hb_prof_begin(k == CBK_COPY ? "k_cbb_copy" : "k_cbb_unfilter", s);
        // (any other kind: CBK_COPY, the last)
        cb_with_kind(k, [&](auto K) { hipLaunchKernelGGL(k_cbb_unfilter<K.value>, dim3(blocks), dim3(256), 0, s, d_frames, d_ufrm + k0, d_ublk + k0, nk, w); });
        hb_prof_end(s);
    }
    hb_prof_begin("k_cbb_finish", s);
    hipLaunchKernelGGL(k_cbb_finish, dim3((unsigned)((nf + 63) / 64)), dim3(64), 0, s, d_frames, (const CbPlan *)d_plans, d_results, (uint32_t)nframes);
    hb_prof_end(s);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}
// ---- many frames, one set of launches (include/hipblosc.h; the host side is hb_cblosc_batch.h) ----
size_t hb_cblosc_decompress_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n) {
    CbbBatch B;
    if (cbb_prepare(nframes, hdrs, nullptr, n, nullptr, nullptr, B, hb_cblosc_accepted())) return 0;
    return B.L.total ? B.L.total : 256;                                   // (never 0 for a batch that is accepted)
}

int hb_cblosc_decompress_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, void *const *d_dst,
                                             const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    if (nframes < 0) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (!hdrs || !d_frame || !n || !d_dst || !cap || !d_work || ((uintptr_t)d_work & 255u) || !d_results) return HB_ERR_BAD_ARG;
    CbbBatch B;
    const int rc = cbb_prepare(nframes, hdrs, d_frame, n, d_dst, cap, B, hb_cblosc_accepted());
    if (rc) return rc;
    const CbbLayout &L = B.L;
    if (work_bytes < L.total) return HB_ERR_SHORT_BUFFER;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    return cbb_launch_batch(nframes, B, (uint8_t *)d_work, d_results, (hipStream_t)stream);
}

// ---- blosc_getitem: items [start, start + nitems) of typesize bytes from the blocks that hold them ----
// Only blocks b_lo .. b_hi are planned, decoded and un-filtered -- whole blocks into a second staging area, then a copy of the range: the
// per-block un-filter kernels (the tile kernels of hb_filters.hip among them) work on whole blocks, and a clipped variant of each would be
// a second set of filters to keep right for at most two partly needed blocks per call.
// (the geometry of a range -- CbRange, cb_getitem_prepare -- is hb_cblosc_getitem_batch.h's, shared with the batch below)

size_t hb_cblosc_getitem_workspace(const hb_cblosc_header *hdr, int64_t start, int64_t nitems) {
    CbRange r;
    if (!hdr || cb_getitem_prepare(hdr, (size_t)hdr->cbytes, start, nitems, r, hb_cblosc_accepted())) return 0;
    return r.total;
}
extern "C++" int hb_cblosc_getitem_prepare(const hb_cblosc_header *hdr, size_t n, int64_t start, int64_t nitems, uint64_t *bytes) {
    CbRange r;
    const int rc = cb_getitem_prepare(hdr, n, start, nitems, r, hb_cblosc_accepted());
    if (!rc) *bytes = r.bytes;
    return rc;
}

int hb_cblosc_getitem_device(const hb_cblosc_header *hdr, const void *d_frame, size_t n, int64_t start, int64_t nitems, void *d_dst, size_t cap,
                             void *d_work, size_t work_bytes, hb_result *d_result, void *stream) {
    if (!hdr) return HB_ERR_BAD_ARG;
    CbRange r;
    const int rc = cb_getitem_prepare(hdr, n, start, nitems, r, hb_cblosc_accepted());
    if (rc) return rc;
    if ((uint64_t)cap < r.bytes) return HB_ERR_SHORT_BUFFER;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (!d_frame || (!d_dst && r.bytes) || !d_work || ((uintptr_t)d_work & 255u) || !d_result) return HB_ERR_BAD_ARG;
    if (work_bytes < r.total) return HB_ERR_SHORT_BUFFER;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *w = (uint8_t *)d_work;
    CbPlan *plan = (CbPlan *)w;
    hipLaunchKernelGGL(k_cb_init, dim3(1), dim3(1), 0, s, plan);
    if (r.bytes) {
        if (hdr->flags & CB_FLAG_MEMCPY) {
            HB_HIP_TRY(hipMemcpyAsync(d_dst, (const uint8_t *)d_frame + 16 + r.off, r.bytes, hipMemcpyDeviceToDevice, s));
        } else {
            uint8_t *stage1 = w + 256 + r.streams, *stage2 = stage1 + r.stage;
            cb_launch_blocks(hdr, (const uint8_t *)d_frame, n, r.b_lo, r.nb, r.vbytes, stage2, plan, (CbStream *)(w + 256), stage1, s);
            HB_HIP_TRY(hipMemcpyAsync(d_dst, stage2 + (r.off - (uint64_t)r.b_lo * hdr->blocksize), r.bytes, hipMemcpyDeviceToDevice, s));
        }
    }
    hipLaunchKernelGGL(k_cb_result, dim3(1), dim3(1), 0, s, plan, d_result, r.bytes);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}

// The plan and the stream decoders over the block records of a batch (hb_cblosc_getitem_frames_batch_device and hb_cblosc_getbox_frames_batch_device
// build the same records): k_cbg_plan, then one decoder launch per kind that occurs (stages k_cbg_decode_small / k_cbg_decode / k_cbg_decode_blz).
static void cbg_launch_decoders(uint32_t nblk, uint32_t nstreams, uint32_t any_small, uint32_t nsplit_all, uint32_t any_lz4, uint32_t any_blz, uint32_t any_zstd, uint32_t any_zlib, const CbgFrame *d_frames,
                                const CbgBlock *d_blocks, CbPlan *d_plans, const uint32_t *d_str0, CbStream *d_streams, uint8_t *w, hipStream_t s) {
    hb_prof_begin("k_cbg_plan", s);
    hipLaunchKernelGGL(k_cbg_plan, dim3((nblk + 63u) / 64u), dim3(64), 0, s, d_frames, d_blocks, d_plans, nblk, d_streams);
    hb_prof_end(s);
    cb_launch_streams(CbgSpace{d_frames, d_blocks, d_plans, d_str0, nblk, w}, d_streams, nstreams, any_small, any_lz4, any_blz, any_zstd, any_zlib, nsplit_all,
                      "k_cbg_decode_small", "k_cbg_decode", "k_cbg_decode_blz", "k_cbg_decode_zstd", "k_cbg_decode_zlib", s);
}

// ---- many ranges of many frames, one set of launches (include/hipblosc.h; the host side is hb_cblosc_getitem_batch.h) ----
size_t hb_cblosc_getitem_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_getitem_job *jobs) {
    return cbg_workspace(nframes, hdrs, n, njobs, jobs, hb_cblosc_accepted());
}

int hb_cblosc_getitem_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_getitem_job *jobs,
                                          void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!hdrs || !d_frame || !n || !jobs || !d_dst || !cap || !d_work || ((uintptr_t)d_work & 255u) || !d_results) return HB_ERR_BAD_ARG;
    CbgBatch B;
    const unsigned accept = hb_cblosc_accepted();
    const int rc = cbg_prepare(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, true, B, accept);
    if (rc) return rc;
    const CbgLayout &L = B.L;
    // (the query knows no capacities and no pointers: where a job was refused for one of them it has counted blocks that this batch leaves out)
    if (work_bytes < (B.ptr_refusals ? cbg_workspace(nframes, hdrs, n, njobs, jobs, accept) : L.total)) return HB_ERR_SHORT_BUFFER;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *w = (uint8_t *)d_work;
    // the records, the prefixes and the cleared plans go up in one copy (the buffer is read before the call returns, as with hb_batch.hip's)
    std::vector<uint8_t> up(L.upload, 0);
    cb_put(up, L.frames, B.frames); cb_put(up, L.jobs, B.jobs); cb_put(up, L.blocks, B.blocks); cb_put(up, L.str0, B.str0);
    cb_put(up, L.gjob, B.gjob); cb_put(up, L.gblk, B.gblk);
    hb_prof_begin("cbg_upload", s);
    HB_HIP_TRY(hipMemcpyAsync(w, up.data(), L.upload, hipMemcpyHostToDevice, s));
    hb_prof_end(s);
    const CbgFrame *d_frames = cb_at<const CbgFrame>(w, L.frames);
    const CbgJob *d_jobs = cb_at<const CbgJob>(w, L.jobs);
    const CbgBlock *d_blocks = cb_at<const CbgBlock>(w, L.blocks);
    CbPlan *d_plans = cb_at<CbPlan>(w, L.plans);
    const uint32_t *d_gjob = cb_at<const uint32_t>(w, L.gjob), *d_gblk = cb_at<const uint32_t>(w, L.gblk);
    if (B.nstreams)
        cbg_launch_decoders((uint32_t)B.nblk, (uint32_t)B.nstreams, B.any_small, B.nsplit_all, B.any_lz4, B.any_blz, B.any_zstd, B.any_zlib, d_frames, d_blocks, d_plans, cb_at<const uint32_t>(w, L.str0),
                            cb_at<CbStream>(w, L.streams), w, s);
    static const char *const gname[CBG_COUNT] = {"k_cbg_gather_copy", "k_cbg_gather_unshuffle", "k_cbg_gather_bitun", "k_cbg_gather_bitun4"};
    cb_launch_kinds(B.kind0, B.kblocks, gname, s, [&](auto K, uint32_t k0, uint32_t nk, uint32_t blocks) {
        hipLaunchKernelGGL(k_cbg_gather<K.value>, dim3(blocks), dim3(256), 0, s, d_frames, d_jobs, d_blocks, (const CbPlan *)d_plans, d_gjob + k0, d_gblk + k0, nk, (const uint8_t *)w);
    });
    hb_prof_begin("k_cbg_finish", s);
    hipLaunchKernelGGL(k_cbg_finish, dim3(((unsigned)njobs + 63u) / 64u), dim3(64), 0, s, d_jobs, (const CbPlan *)d_plans, d_results, (uint32_t)njobs);
    hb_prof_end(s);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}

// A prepared batch of boxes, of stepped selections, of index-list selections or of points (CbxBatch) on the device: one upload, the plan and the
// decoders over the distinct blocks, the gathers -- k_cbx_gather per kind among the jobs with plain rows, k_cbs_gather per kind among those with
// stepped rows, k_cbi_gather_rows and k_cbi_gather_items per kind among those with an index list, k_cbp_gather per kind among the jobs of
// points -- and the records.  d_sel_tab: the point table of a prepared selection, which the point gather then reads in place of the batch's own
// (whose section of the layout is empty).
static int cbx_launch(const CbxBatch &B, int njobs, void *d_work, hb_result *d_results, void *stream, const CbpPoint *d_sel_tab = nullptr) {
    const CbxLayout &L = B.L;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *w = (uint8_t *)d_work;
    // the records, the touch lists, the prefixes and the cleared plans go up in one copy (the buffer is read before the call returns)
    std::vector<uint8_t> up(L.upload, 0);
    cb_put(up, L.frames, B.frames); cb_put(up, L.jobs, B.jobs); cb_put(up, L.blocks, B.blocks); cb_put(up, L.str0, B.str0); cb_put(up, L.touch, B.touch);
    cb_put(up, L.gjob, B.gjob); cb_put(up, L.gblk, B.gblk);
    cb_put(up, L.srow, B.srow); cb_put(up, L.sgjob, B.sgjob); cb_put(up, L.sgblk, B.sgblk);
    cb_put(up, L.irow, B.irow); cb_put(up, L.igjob, B.igjob); cb_put(up, L.igblk, B.igblk); cb_put(up, L.itab, B.itab);
    cb_put(up, L.prow, B.prow); cb_put(up, L.pgjob, B.pgjob); cb_put(up, L.pgblk, B.pgblk); cb_put(up, L.ptab, B.ptab);
    hb_prof_begin("cbx_upload", s);
    HB_HIP_TRY(hipMemcpyAsync(w, up.data(), L.upload, hipMemcpyHostToDevice, s));
    hb_prof_end(s);
    const CbgFrame *d_frames = cb_at<const CbgFrame>(w, L.frames);
    const CbxJob *d_jobs = cb_at<const CbxJob>(w, L.jobs);
    const CbgBlock *d_blocks = cb_at<const CbgBlock>(w, L.blocks);
    CbPlan *d_plans = cb_at<CbPlan>(w, L.plans);
    const CbxTouch *d_touch = cb_at<const CbxTouch>(w, L.touch);
    if (B.nstreams)
        cbg_launch_decoders((uint32_t)B.nblk, (uint32_t)B.nstreams, B.any_small, B.nsplit_all, B.any_lz4, B.any_blz, B.any_zstd, B.any_zlib, d_frames, d_blocks, d_plans, cb_at<const uint32_t>(w, L.str0),
                            cb_at<CbStream>(w, L.streams), w, s);
    const uint32_t *d_gjob = cb_at<const uint32_t>(w, L.gjob), *d_gblk = cb_at<const uint32_t>(w, L.gblk);
    static const char *const gname[CBG_COUNT] = {"k_cbx_gather_copy", "k_cbx_gather_unshuffle", "k_cbx_gather_bitun", "k_cbx_gather_bitun4"};
    cb_launch_kinds(B.kind0, B.kblocks, gname, s, [&](auto K, uint32_t k0, uint32_t nk, uint32_t blocks) {
        hipLaunchKernelGGL(k_cbx_gather<K.value>, dim3(blocks), dim3(256), 0, s, d_frames, d_jobs, d_blocks, (const CbPlan *)d_plans, d_touch, d_gjob + k0, d_gblk + k0, nk,
                           (const uint8_t *)w);
    });
    const CbsRow *d_srow = cb_at<const CbsRow>(w, L.srow);
    const uint32_t *d_sgjob = cb_at<const uint32_t>(w, L.sgjob), *d_sgblk = cb_at<const uint32_t>(w, L.sgblk);
    static const char *const sname[CBG_COUNT] = {"k_cbs_gather_copy", "k_cbs_gather_unshuffle", "k_cbs_gather_bitun", "k_cbs_gather_bitun4"};
    cb_launch_kinds(B.skind0, B.skblocks, sname, s, [&](auto K, uint32_t k0, uint32_t nk, uint32_t blocks) {
        hipLaunchKernelGGL(k_cbs_gather<cbr_items_kind(K.value)>, dim3(blocks), dim3(256), 0, s, d_frames, d_jobs, d_srow + k0, d_blocks, (const CbPlan *)d_plans, d_touch,
                           d_sgjob + k0, d_sgblk + k0, nk, (const uint8_t *)w);
    });
    // (the index jobs' launch list: the rows gather's kinds, then the items gather's)
    const CbiRow *d_irow = cb_at<const CbiRow>(w, L.irow);
    const uint32_t *d_igjob = cb_at<const uint32_t>(w, L.igjob), *d_igblk = cb_at<const uint32_t>(w, L.igblk), *d_itab = cb_at<const uint32_t>(w, L.itab);
    static const char *const iname[2 * CBG_COUNT] = {"k_cbi_gather_rows_copy",  "k_cbi_gather_rows_unshuffle",  "k_cbi_gather_rows_bitun",  "k_cbi_gather_rows_bitun4",
                                                     "k_cbi_gather_items_copy", "k_cbi_gather_items_unshuffle", "k_cbi_gather_items_bitun", "k_cbi_gather_items_bitun4"};
    cb_launch_kinds(B.ikind0, B.ikblocks, iname, s, [&](auto K, uint32_t k0, uint32_t nk, uint32_t blocks) {
        hipLaunchKernelGGL(k_cbi_gather_rows<K.value>, dim3(blocks), dim3(256), 0, s, d_frames, d_jobs, d_irow + k0, d_blocks, (const CbPlan *)d_plans, d_touch, d_itab, d_igjob + k0,
                           d_igblk + k0, nk, (const uint8_t *)w);
    });
    cb_launch_kinds(B.ikind0 + CBG_COUNT, B.ikblocks + CBG_COUNT, iname + CBG_COUNT, s, [&](auto K, uint32_t k0, uint32_t nk, uint32_t blocks) {
        hipLaunchKernelGGL(k_cbi_gather_items<cbr_items_kind(K.value)>, dim3(blocks), dim3(256), 0, s, d_frames, d_jobs, d_irow + k0, d_blocks, (const CbPlan *)d_plans, d_touch, d_itab,
                           d_igjob + k0, d_igblk + k0, nk, (const uint8_t *)w);
    });
    const CbpRow *d_prow = cb_at<const CbpRow>(w, L.prow);
    const CbpPoint *d_ptab = d_sel_tab ? d_sel_tab : cb_at<const CbpPoint>(w, L.ptab);
    const uint32_t *d_pgjob = cb_at<const uint32_t>(w, L.pgjob), *d_pgblk = cb_at<const uint32_t>(w, L.pgblk);
    static const char *const pname[CBG_COUNT] = {"k_cbp_gather_copy", "k_cbp_gather_unshuffle", "k_cbp_gather_bitun", "k_cbp_gather_bitun4"};
    cb_launch_kinds(B.pkind0, B.pkblocks, pname, s, [&](auto K, uint32_t k0, uint32_t nk, uint32_t blocks) {
        hipLaunchKernelGGL(k_cbp_gather<cbr_items_kind(K.value)>, dim3(blocks), dim3(256), 0, s, d_frames, d_jobs, d_prow + k0, d_blocks, (const CbPlan *)d_plans, d_touch, d_ptab,
                           d_pgjob + k0, d_pgblk + k0, nk, (const uint8_t *)w);
    });
    hb_prof_begin("k_cbx_finish", s);
    hipLaunchKernelGGL(k_cbx_finish, dim3(((unsigned)njobs + 63u) / 64u), dim3(64), 0, s, d_jobs, (const CbPlan *)d_plans, d_touch, d_results, (uint32_t)njobs);
    hb_prof_end(s);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}
// The three N-d `_device` calls, the point batch's and the prepared selection's read: bad argument, then what `prepare` says, then short buffer,
// then no device; and the launches.  `prepare` fills the batch, `workspace` is the call's own size query, d_sel_tab the prepared selection's table.
extern "C++" {
template <class PREPARE, class WORKSPACE>
static int cbx_device_call(int nframes, int njobs, bool have_all, void *d_work, size_t work_bytes, hb_result *d_results, void *stream, PREPARE prepare,
                           WORKSPACE workspace, const CbpPoint *d_sel_tab = nullptr) {
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!have_all || !d_work || ((uintptr_t)d_work & 255u) || !d_results) return HB_ERR_BAD_ARG;
    CbxBatch B;
    const unsigned accept = hb_cblosc_accepted();
    const int rc = prepare(B, accept);
    if (rc) return rc;
    // (the query knows no capacities and no pointers: where a job was refused for one of them it has counted blocks that this batch leaves out)
    if (work_bytes < (B.ptr_refusals ? workspace(accept) : B.L.total)) return HB_ERR_SHORT_BUFFER;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    return cbx_launch(B, njobs, d_work, d_results, stream, d_sel_tab);
}
}

// ---- many boxes of many frames, one set of launches (include/hipblosc.h; the host side is hb_cblosc_box_batch.h) ----
size_t hb_cblosc_getbox_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_box_job *jobs) {
    return cbx_workspace(nframes, hdrs, n, njobs, jobs, hb_cblosc_accepted());
}

int hb_cblosc_getbox_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_box_job *jobs,
                                         void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    return cbx_device_call(
        nframes, njobs, hdrs && d_frame && n && jobs && d_dst && cap, d_work, work_bytes, d_results, stream,
        [&](CbxBatch &B, unsigned accept) { return cbx_prepare(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, true, B, accept); },
        [&](unsigned accept) { return cbx_workspace(nframes, hdrs, n, njobs, jobs, accept); });
}

// ---- many stepped selections of many frames, one set of launches (include/hipblosc.h; the host side is hb_cblosc_slice_batch.h) ----
size_t hb_cblosc_getslice_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_slice_job *jobs) {
    return cbs_workspace(nframes, hdrs, n, njobs, jobs, hb_cblosc_accepted());
}

int hb_cblosc_getslice_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_slice_job *jobs,
                                           void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    return cbx_device_call(
        nframes, njobs, hdrs && d_frame && n && jobs && d_dst && cap, d_work, work_bytes, d_results, stream,
        [&](CbxBatch &B, unsigned accept) { return cbs_prepare(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, true, B, accept); },
        [&](unsigned accept) { return cbs_workspace(nframes, hdrs, n, njobs, jobs, accept); });
}

// ---- many orthogonal selections of many frames, one set of launches (include/hipblosc.h; the host side is hb_cblosc_index_batch.h) ----
size_t hb_cblosc_getindex_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_index_job *jobs, const int64_t *index,
                                                 int64_t nindex) {
    return cbi_workspace(nframes, hdrs, n, njobs, jobs, index, nindex, hb_cblosc_accepted());
}

int hb_cblosc_getindex_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_index_job *jobs,
                                           const int64_t *index, int64_t nindex, void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results,
                                           void *stream) {
    return cbx_device_call(
        nframes, njobs, hdrs && d_frame && n && jobs && d_dst && cap, d_work, work_bytes, d_results, stream,
        [&](CbxBatch &B, unsigned accept) { return cbi_prepare(nframes, hdrs, d_frame, n, njobs, jobs, index, nindex, d_dst, cap, true, B, accept); },
        [&](unsigned accept) { return cbi_workspace(nframes, hdrs, n, njobs, jobs, index, nindex, accept); });
}

// ---- many coordinate selections of many frames, one set of launches (include/hipblosc.h; the host side is hb_cblosc_point_batch.h) ----
size_t hb_cblosc_getpoints_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points,
                                                  int64_t npoints) {
    return cbp_workspace(nframes, hdrs, n, njobs, jobs, points, npoints, hb_cblosc_accepted());
}

int hb_cblosc_getpoints_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_point_job *jobs,
                                            const hb_cblosc_point *points, int64_t npoints, void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes,
                                            hb_result *d_results, void *stream) {
    return cbx_device_call(
        nframes, njobs, hdrs && d_frame && n && jobs && d_dst && cap, d_work, work_bytes, d_results, stream,
        [&](CbxBatch &B, unsigned accept) { return cbp_prepare(nframes, hdrs, d_frame, n, njobs, jobs, points, npoints, d_dst, cap, true, B, accept); },
        [&](unsigned accept) { return cbp_workspace(nframes, hdrs, n, njobs, jobs, points, npoints, accept); });
}

size_t hb_cblosc_bound(size_t n, int typesize) {
    return cbe_bound(n, typesize);
}
size_t hb_cblosc_compress_workspace(size_t n, int shuffle, int typesize) { return cbe_layout(n, shuffle, typesize > 0 ? typesize : 1).total; }

// shuffle: 0 none, 1 byte shuffle, 2 bit shuffle (c-blosc's BLOSC_NOSHUFFLE / BLOSC_SHUFFLE / BLOSC_BITSHUFFLE).  Asynchronous on `stream`.
int hb_cblosc_compress_dev(const void *d_src, size_t n, void *d_frame, size_t cap, int shuffle, int typesize, void *d_work, size_t work_bytes,
                           hb_result *d_result, void *stream) {
    const CbMatcher M = cb_matcher(hb_cblosc_policy());                   // (read once: one call, one policy)
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if ((!d_src && n) || !d_frame || !d_work || ((uintptr_t)d_work & 255u) || !d_result) return HB_ERR_BAD_ARG;
    if (typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    if (n > 0x7FFFFFFFull - 64u * 1024u * 1024u) return HB_ERR_DATA_TOO_LARGE;           // (c-blosc: BLOSC_MAX_BUFFERSIZE = INT_MAX - 16)
    if (cap < hb_cblosc_bound(n, typesize)) return HB_ERR_SHORT_BUFFER;
    const CbEncLayout L = cbe_layout(n, shuffle, typesize);
    if (work_bytes < L.total) return HB_ERR_SHORT_BUFFER;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *w = (uint8_t *)d_work;
    CbEncPlan *plan = (CbEncPlan *)(w + L.plan);
    uint32_t *tiles = (uint32_t *)(w + L.tiles);
    CbChunkDesc *desc = (CbChunkDesc *)(w + L.desc);
    uint8_t *records = w + L.records, *filtered = w + L.filtered;
    const bool unshuf = shuffle == 1 && typesize > 1, bits = shuffle == 2;
    const bool memcpyed = n < HB_CHUNK || M.store;                        // (such a frame names LZ4 under either stream format, as it always did)
    const uint32_t flags = (unshuf ? CB_FLAG_SHUFFLE : 0u) | (bits ? CB_FLAG_BITSHUFFLE : 0u) | (L.nsplit == 1u ? CB_FLAG_DONTSPLIT : 0u) |
                           (M.zstd && !memcpyed ? CB_FLAGS_ZSTD : CB_FLAGS_LZ4);
    if (memcpyed) {                                        // (level 0: blosc_compress's memcpyed frame, at every size)
        if (n) HB_HIP_TRY(hipMemcpyAsync((uint8_t *)d_frame + 16, d_src, n, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_cbe_memcpy_header, dim3(1), dim3(1), 0, s, (uint8_t *)d_frame, (uint32_t)n, (uint32_t)typesize, flags | CB_FLAG_MEMCPY | CB_FLAG_DONTSPLIT, d_result);
        HB_HIP_TRY(hipGetLastError());
        return HB_OK;
    }
    const uint8_t *fsrc = (const uint8_t *)d_src;
    // the fused shuffle + match route (cbe_fuse, hb_cblosc_enc_batch.h): no filtered buffer, except for the last, shorter block
    const bool fuse = cbe_fuse(cbe_geom(n, shuffle, typesize), typesize, d_src);
    const uint32_t tail = (uint32_t)(n - (size_t)L.nfull * L.blocksize);
    hb_prof_begin("k_cb_filter", s);
    if (fuse) {
        if (tail) hipLaunchKernelGGL(k_cb_shuffle, dim3(64), dim3(256), 0, s, filtered + (size_t)L.nfull * L.blocksize, (const uint8_t *)d_src + (size_t)L.nfull * L.blocksize, tail, L.blocksize, (uint32_t)typesize);
    } else if (unshuf || bits) {
        if (unshuf) {
            if (hb_launch_shuffle_blocks(false, filtered, (const uint8_t *)d_src, L.nfull, L.blocksize, typesize, s)) {
                if (tail) hipLaunchKernelGGL(k_cb_shuffle, dim3(64), dim3(256), 0, s, filtered + (size_t)L.nfull * L.blocksize, (const uint8_t *)d_src + (size_t)L.nfull * L.blocksize, tail, L.blocksize, (uint32_t)typesize);
            } else hipLaunchKernelGGL(k_cb_shuffle, dim3(2048), dim3(256), 0, s, filtered, (const uint8_t *)d_src, (uint32_t)n, L.blocksize, (uint32_t)typesize);
        }
        else if (typesize == 4 && L.blocksize % 512u == 0u && L.nfull) {
            hipLaunchKernelGGL(k_cb_bitshuffle4_fast<true>, dim3(cb_grid((uint64_t)L.nfull * (L.blocksize / 128u))), dim3(256), 0, s, filtered, (const uint8_t *)d_src, L.nfull, L.blocksize);
            if (tail) hipLaunchKernelGGL(k_cb_bitshuffle, dim3(64), dim3(256), 0, s, filtered + (size_t)L.nfull * L.blocksize, (const uint8_t *)d_src + (size_t)L.nfull * L.blocksize, tail, L.blocksize, (uint32_t)typesize);
        } else hipLaunchKernelGGL(k_cb_bitshuffle, dim3(2048), dim3(256), 0, s, filtered, (const uint8_t *)d_src, (uint32_t)n, L.blocksize, (uint32_t)typesize);
        fsrc = filtered;
    }
    hb_prof_end(s);
    HB_HIP_TRY(hipMemsetAsync(plan, 0, sizeof(CbEncPlan), s));
    const uint32_t fused_nblk = fuse ? L.nfull : 0u;
    if (L.nchunks) {
        hb_prof_begin("k_match", s);
        if (fuse) hb_launch_match_fused_selfcontained((const uint8_t *)d_src, typesize, desc, records, L.nfull, M.ways, M.accel, s);
        else hb_launch_match_selfcontained(fsrc, (size_t)L.nchunks * HB_CHUNK, desc, records, L.nchunks, M.ways, M.accel, s);
        hb_prof_end(s);
        if (M.zstd) cbe_zstd_stage(nullptr, nullptr, 0u, L.nchunks, desc, records, fsrc, L.nchunks, L.nsplit, fused_nblk, s);
        hb_prof_begin("k_cbe_pack", s);
        hipLaunchKernelGGL(k_cbe_tiles, dim3(L.ntiles), dim3(256), 0, s, desc, L.nchunks, L.nsplit, fused_nblk, tiles);
        hipLaunchKernelGGL(k_cbe_scan, dim3(1), dim3(1024), 0, s, tiles, L.ntiles, plan);
        hipLaunchKernelGGL(k_cbe_pack, dim3(L.ntiles), dim3(1024), 0, s, desc, records, fsrc, tiles, L.nchunks, L.nsplit, fused_nblk, 16u + 4u * L.nblocks, (uint8_t *)d_frame);
        hb_prof_end(s);
    }
    hipLaunchKernelGGL(k_cbe_finish, dim3(1), dim3(64), 0, s, plan, fuse ? (const uint8_t *)filtered : fsrc, (uint32_t)n, L.blocksize, (uint32_t)typesize, flags, L.nfull, 16u + 4u * L.nblocks, (uint8_t *)d_frame,
                       (uint64_t)cap, d_result);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}
// everything of a batched encode behind cbe_prepare: upload, map, filter, matchers, tiles, scan, pack, finish over the workspace `w` that B was
// laid out for.  Every batched writer ends here, with the policy word its entry point read.  Level 0: every frame that would have gone to a
// matcher is memcpyed instead, as hb_cblosc_compress_dev writes it -- the frame records change their route on their way up, nothing but the
// upload and k_cbeb_finish is launched (one wavefront copies a frame: chunk-sized frames), and the layout, made for the matchers, is more
// than enough.
static int cbe_launch_batch(int nframes, const CbeBatch &B, int shuffle, int typesize, unsigned policy, uint8_t *w, hb_result *d_results, hipStream_t s) {
    const CbeLayout &L = B.L;
    const size_t nf = (size_t)nframes;
    const CbMatcher M = cb_matcher(policy);
    // the frame records, the matcher's records, the prefixes and the cleared plans go up in one copy (the buffer is read before the call returns)
    std::vector<uint8_t> up(L.upload, 0);
    memcpy(up.data() + L.frames, B.tab.data(), nf * sizeof(CbeFrame));
    if (M.store) {
        CbeFrame *t = (CbeFrame *)(up.data() + L.frames);
        for (size_t k = 0; k < nf; k++)
            if (t[k].mode == CBE_PLAIN || t[k].mode == CBE_FUSED) { t[k].mode = CBE_MEMCPY; t[k].flags |= CB_FLAG_MEMCPY | CB_FLAG_DONTSPLIT; }
    }
    if (M.zstd) {                                                         // (the frames that go through the matcher: their headers name the streams' format)
        CbeFrame *t = (CbeFrame *)(up.data() + L.frames);
        for (size_t k = 0; k < nf; k++)
            if (t[k].mode == CBE_PLAIN || t[k].mode == CBE_FUSED) t[k].flags = (t[k].flags & ~0xE0u) | CB_FLAGS_ZSTD;
    }
    memcpy(up.data() + L.bf, B.bf.data(), nf * sizeof(BatchFrame));
    memcpy(up.data() + L.pre, B.pre.data(), nf * 8);
    memcpy(up.data() + L.plans, B.plans.data(), nf * sizeof(CbEncPlan));
    hb_prof_begin("cbeb_upload", s);
    HB_HIP_TRY(hipMemcpyAsync(w, up.data(), L.upload, hipMemcpyHostToDevice, s));
    hb_prof_end(s);
    const CbeFrame *d_frames = (const CbeFrame *)(w + L.frames);
    const BatchFrame *d_bf = (const BatchFrame *)(w + L.bf);
    const uint32_t *d_tile0 = (const uint32_t *)(w + L.pre), *d_fblk = d_tile0 + nf;
    CbEncPlan *d_plans = (CbEncPlan *)(w + L.plans);
    uint32_t *d_map = (uint32_t *)(w + L.map), *d_tiles = (uint32_t *)(w + L.tiles);
    CbChunkDesc *d_desc = (CbChunkDesc *)(w + L.desc);
    uint8_t *d_records = w + L.records;
    const uint32_t plain = M.store ? 0u : (uint32_t)B.plain_chunks, fused = M.store ? 0u : (uint32_t)B.fused_chunks, ntiles = M.store ? 0u : (uint32_t)B.ntiles;
    if (B.map_chunks && !M.store) {
        hb_prof_begin("k_cbeb_map", s);
        hipLaunchKernelGGL(k_cbeb_map, dim3((unsigned)nframes), dim3(64), 0, s, d_frames, d_map);
        hb_prof_end(s);
    }
    if (B.fblocks && !M.store) {
        hb_prof_begin("k_cbeb_filter", s);
        if (shuffle == 2) hipLaunchKernelGGL(k_cbeb_filter<true>, dim3((unsigned)B.fblocks), dim3(256), 0, s, d_frames, d_fblk, (uint32_t)nframes, w);
        else hipLaunchKernelGGL(k_cbeb_filter<false>, dim3((unsigned)B.fblocks), dim3(256), 0, s, d_frames, d_fblk, (uint32_t)nframes, w);
        hb_prof_end(s);
    }
    if (fused) {
        hb_prof_begin("k_match_fused", s);
        hb_launch_match_fused_selfcontained_batch(d_bf, d_map, typesize, d_desc + plain, d_records + (size_t)plain * HB_RSTRIDE, fused, M.ways, M.accel, s);
        hb_prof_end(s);
    }
    if (plain) {
        hb_prof_begin("k_match", s);
        // with a filter the whole blocks of these frames lie chunk after chunk in one area: one long buffer of self-contained chunks, no map
        if (B.filtered) hb_launch_match_selfcontained(w + L.filt, (size_t)plain * HB_CHUNK, d_desc, d_records, plain, M.ways, M.accel, s);
        else hb_launch_match_selfcontained_batch(d_bf, d_map, d_desc, d_records, plain, M.ways, M.accel, s);
        hb_prof_end(s);
    }
    if (ntiles && M.zstd) cbe_zstd_stage(d_frames, d_tile0, (uint32_t)nframes, ntiles * 1024u, d_desc, d_records, w, 0u, 0u, 0u, s);
    if (ntiles) {
        hb_prof_begin("k_cbeb_tiles", s);
        hipLaunchKernelGGL(k_cbeb_tiles, dim3(ntiles), dim3(256), 0, s, d_frames, d_tile0, (uint32_t)nframes, (const CbChunkDesc *)d_desc, d_tiles);
        hb_prof_end(s);
        hb_prof_begin("k_cbeb_scan", s);
        hipLaunchKernelGGL(k_cbeb_scan, dim3((unsigned)nframes), dim3(1024), 0, s, d_frames, d_tiles, d_plans);
        hb_prof_end(s);
        hb_prof_begin("k_cbeb_pack", s);
        hipLaunchKernelGGL(k_cbeb_pack, dim3(ntiles), dim3(1024), 0, s, d_frames, d_tile0, (uint32_t)nframes, (const CbChunkDesc *)d_desc, (const uint8_t *)d_records,
                           (const uint32_t *)d_tiles, (const uint8_t *)w);
        hb_prof_end(s);
    }
    hb_prof_begin("k_cbeb_finish", s);
    hipLaunchKernelGGL(k_cbeb_finish, dim3((unsigned)nframes), dim3(64), 0, s, d_frames, (const CbEncPlan *)d_plans, (const uint8_t *)w, d_results);
    hb_prof_end(s);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}
// ---- many inputs, one set of launches (include/hipblosc.h; the host side is hb_cblosc_enc_batch.h) ----
size_t hb_cblosc_compress_frames_batch_workspace(int nframes, const size_t *n, int shuffle, int typesize) {
    CbeBatch B;
    if (cbe_prepare(nframes, nullptr, n, nullptr, nullptr, shuffle, typesize, nullptr, B)) return 0;
    return B.query;
}

int hb_cblosc_compress_frames_batch_device(int nframes, const void *const *d_src, const size_t *n, void *const *d_frame, const size_t *cap, int shuffle, int typesize,
                                           void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    const unsigned policy = hb_cblosc_policy();                           // (hb_cblosc_set_compressor, read once: one call, one policy)
    if (nframes < 0 || typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (!d_src || !n || !d_frame || !cap || !d_work || ((uintptr_t)d_work & 255u) || !d_results) return HB_ERR_BAD_ARG;
    uint8_t *w = (uint8_t *)d_work;
    CbeBatch B;
    const int rc = cbe_prepare(nframes, d_src, n, d_frame, cap, shuffle, typesize, w, B);
    if (rc) return rc;
    const CbeLayout &L = B.L;
    if (work_bytes < B.query || B.query < L.total) return HB_ERR_SHORT_BUFFER;      // (the layout never exceeds the query: hb_cblosc_enc_batch.h)
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    return cbe_launch_batch(nframes, B, shuffle, typesize, policy, w, d_results, (hipStream_t)stream);
}

// ---- many source boxes, one set of launches (include/hipblosc.h; the host side is hb_cblosc_enc_box_batch.h) ----
size_t hb_cblosc_compress_boxes_batch_workspace(int nframes, const hb_cblosc_src_box *boxes, int shuffle, int typesize) {
    return cbxe_workspace(nframes, boxes, shuffle, typesize);
}

int hb_cblosc_compress_boxes_batch_device(int nframes, const hb_cblosc_src_box *boxes, const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill,
                                          int shuffle, int typesize, void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    const unsigned policy = hb_cblosc_policy();                           // (hb_cblosc_set_compressor, read once: one call, one policy)
    if (nframes < 0 || typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (!boxes || !d_src || !d_frame || !cap || !d_work || ((uintptr_t)d_work & 255u) || !d_results) return HB_ERR_BAD_ARG;
    uint8_t *w = (uint8_t *)d_work;
    CbxeBatch B;
    const int rc = cbxe_prepare(nframes, boxes, d_src, d_frame, cap, fill, shuffle, typesize, w, B);
    if (rc) return rc;
    const CbxeLayout &L = B.L;
    // (the query knows no pointers: it stages every frame, so this layout never exceeds it -- as the encoder's own never exceeds its query)
    const size_t query = cbxe_workspace(nframes, boxes, shuffle, typesize);
    if (!query) return HB_ERR_BAD_ARG;                                    // (the limits are taken as the query takes them: over all frames as if every one were staged)
    if (work_bytes < query || query < L.total || B.E.query < B.E.L.total) return HB_ERR_SHORT_BUFFER;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const size_t nj = B.jobs.size();
    // the job records, their workgroup prefix and the fill table go up in one copy (the buffer is read before the call returns)
    std::vector<uint8_t> up(L.upload, 0);
    if (nj) memcpy(up.data() + L.jobs, B.jobs.data(), nj * sizeof(CbxeJob));
    memcpy(up.data() + L.gblk, B.gblk.data(), (nj + 1) * 4);
    memcpy(up.data() + L.fill, B.table, CBXE_FILL_BYTES);
    hb_prof_begin("cbxe_upload", s);
    HB_HIP_TRY(hipMemcpyAsync(w, up.data(), L.upload, hipMemcpyHostToDevice, s));
    hb_prof_end(s);
    if (nj) {
        hb_prof_begin("k_cbxe_gather", s);
        hipLaunchKernelGGL(k_cbxe_gather, dim3((unsigned)B.groups), dim3(256), 0, s, (const CbxeJob *)(w + L.jobs), (const uint32_t *)(w + L.gblk), (uint32_t)nj,
                           (const uint8_t *)(w + L.fill), (uint32_t)typesize, cbx_recip((uint32_t)typesize));
        hb_prof_end(s);
    }
    return cbe_launch_batch(nframes, B.E, shuffle, typesize, policy, w + L.enc, d_results, s);
}

// ---- the update batches: boxes, selections, points and prepared point selections go one way.  Each is the box updates' batch (CbxuBatch: fill
// bases, old-frame bases, the encoder) plus a stage that puts the source's items over the staged bases. ----
// A prepared update batch on the device: one upload under `label` (the stage's records by `put`, the finish list, and behind them the gather's
// records, prefix and fill table: the buffer is read before the call returns), the fill bases and the whole chunks that are not read where
// they lie, the old-frame bases straight into their staged slots, the stage's launches by `scatter`, the encoder and the records.
extern "C++" {
template <class PUT, class SCATTER>
static int cbu_launch(const CbxuBatch &B, int njobs, int shuffle, int typesize, unsigned policy, uint8_t *w, hb_result *d_results, hipStream_t s, const char *label, PUT put,
                      SCATTER scatter) {
    const CbxuLayout &L = B.L;
    const CbxeLayout &XL = B.X.L;
    const size_t ng = B.X.jobs.size(), nd = B.fin.size();
    std::vector<uint8_t> up(L.box + XL.upload, 0);
    put(up.data());
    if (nd) memcpy(up.data() + L.fin, B.fin.data(), nd * 4);
    if (ng) memcpy(up.data() + L.box + XL.jobs, B.X.jobs.data(), ng * sizeof(CbxeJob));
    memcpy(up.data() + L.box + XL.gblk, B.X.gblk.data(), (ng + 1) * 4);
    memcpy(up.data() + L.box + XL.fill, B.X.table, CBXE_FILL_BYTES);
    hb_prof_begin(label, s);
    HB_HIP_TRY(hipMemcpyAsync(w, up.data(), up.size(), hipMemcpyHostToDevice, s));
    hb_prof_end(s);
    uint8_t *wx = w + L.box;
    hb_result *d_dres = (hb_result *)(w + L.dres);
    if (ng) {
        hb_prof_begin("k_cbxe_gather", s);
        hipLaunchKernelGGL(k_cbxe_gather, dim3((unsigned)B.ggroups), dim3(256), 0, s, (const CbxeJob *)(wx + XL.jobs), (const uint32_t *)(wx + XL.gblk), (uint32_t)ng,
                           (const uint8_t *)(wx + XL.fill), (uint32_t)typesize, cbx_recip((uint32_t)typesize));
        hb_prof_end(s);
    }
    if (nd) {
        const int st = cbb_launch_batch((int)nd, B.D, w + L.dec, d_dres, s);
        if (st) return st;
    }
    scatter(w, s);
    // (the encoder reads the staged bytes of a base that failed to decode: they lie inside the workspace and may be anything, and the encoder
    // takes any bytes; k_cbxu_finish then overrides that frame's record)
    const int st = cbe_launch_batch(njobs, B.X.E, shuffle, typesize, policy, wx + XL.enc, d_results, s);
    if (st) return st;
    if (nd) {
        hb_prof_begin("k_cbxu_finish", s);
        hipLaunchKernelGGL(k_cbxu_finish, dim3((unsigned)((nd + 63) / 64)), dim3(64), 0, s, (const uint32_t *)(w + L.fin), (const hb_result *)d_dres, d_results, (uint32_t)nd);
        hb_prof_end(s);
        HB_HIP_TRY(hipGetLastError());
    }
    return HB_OK;
}
}
// the stages: the box updates' overlay, the selection updates' two scatters, the point updates' scatter
static int cbxu_launch(const CbxuBatch &B, int njobs, int shuffle, int typesize, unsigned policy, uint8_t *w, hb_result *d_results, void *stream) {
    const CbxuLayout &L = B.L;
    const size_t no = B.jobs.size();
    return cbu_launch(
        B, njobs, shuffle, typesize, policy, w, d_results, (hipStream_t)stream, "cbxu_upload",
        [&](uint8_t *up) {
            if (no) { memcpy(up + L.jobs, B.jobs.data(), no * sizeof(CbxuJob)); memcpy(up + L.oblk, B.oblk.data(), (no + 1) * 4); }
        },
        [&](uint8_t *w, hipStream_t s) {
            if (!no) return;
            hb_prof_begin("k_cbxu_overlay", s);
            hipLaunchKernelGGL(k_cbxu_overlay, dim3((unsigned)B.ogroups), dim3(256), 0, s, (const CbxuJob *)(w + L.jobs), (const uint32_t *)(w + L.oblk), (uint32_t)no);
            hb_prof_end(s);
        });
}
static int cbiu_launch(const CbiuBatch &B, int njobs, int shuffle, int typesize, unsigned policy, uint8_t *w, hb_result *d_results, void *stream) {
    const CbiuLayout &SL = B.S;
    const size_t sel = B.U.L.sel, nr = B.rjobs.size(), ni = B.ijobs.size(), nt = B.tab.size();
    return cbu_launch(
        B.U, njobs, shuffle, typesize, policy, w, d_results, (hipStream_t)stream, "cbiu_upload",
        [&](uint8_t *up) {
            uint8_t *us = up + sel;
            if (nr) { memcpy(us + SL.rjobs, B.rjobs.data(), nr * sizeof(CbiuJob)); memcpy(us + SL.rblk, B.rblk.data(), (nr + 1) * 4); }
            if (ni) { memcpy(us + SL.ijobs, B.ijobs.data(), ni * sizeof(CbiuJob)); memcpy(us + SL.iblk, B.iblk.data(), (ni + 1) * 4); }
            if (nt) memcpy(us + SL.tab, B.tab.data(), nt * sizeof(CbiuPair));
        },
        [&](uint8_t *w, hipStream_t s) {
            uint8_t *ws = w + sel;
            if (nr) {
                hb_prof_begin("k_cbiu_scatter_rows", s);
                hipLaunchKernelGGL(k_cbiu_scatter_rows, dim3((unsigned)B.rgroups), dim3(256), 0, s, (const CbiuJob *)(ws + SL.rjobs), (const uint32_t *)(ws + SL.rblk), (uint32_t)nr,
                                   (const CbiuPair *)(ws + SL.tab));
                hb_prof_end(s);
            }
            if (ni) {
                hb_prof_begin("k_cbiu_scatter_items", s);
                hipLaunchKernelGGL(k_cbiu_scatter_items, dim3((unsigned)B.igroups), dim3(256), 0, s, (const CbiuJob *)(ws + SL.ijobs), (const uint32_t *)(ws + SL.iblk), (uint32_t)ni,
                                   (const CbiuPair *)(ws + SL.tab), (uint32_t)typesize);
                hb_prof_end(s);
            }
        });
}
// (d_sel_tab: the point table of a prepared selection, which the scatter then reads in place of the batch's own -- none is uploaded)
static int cbpu_launch(const CbpuBatch &B, int njobs, const CbpPoint *d_sel_tab, int shuffle, int typesize, unsigned policy, uint8_t *w, hb_result *d_results, void *stream) {
    const CbpuLayout &SL = B.S;
    const size_t sel = B.U.L.sel, np = B.jobs.size(), nt = B.tab.size();
    return cbu_launch(
        B.U, njobs, shuffle, typesize, policy, w, d_results, (hipStream_t)stream, "cbpu_upload",
        [&](uint8_t *up) {
            uint8_t *us = up + sel;
            if (np) { memcpy(us + SL.jobs, B.jobs.data(), np * sizeof(CbpuJob)); memcpy(us + SL.blk, B.blk.data(), (np + 1) * 4); }
            if (nt) memcpy(us + SL.tab, B.tab.data(), nt * sizeof(CbpPoint));
        },
        [&](uint8_t *w, hipStream_t s) {
            if (!np) return;
            uint8_t *ws = w + sel;
            hb_prof_begin("k_cbpu_scatter_points", s);
            hipLaunchKernelGGL(k_cbpu_scatter_points, dim3((unsigned)B.groups), dim3(256), 0, s, (const CbpuJob *)(ws + SL.jobs), (const uint32_t *)(ws + SL.blk), (uint32_t)np,
                               d_sel_tab ? d_sel_tab : (const CbpPoint *)(ws + SL.tab), (uint32_t)typesize);
            hb_prof_end(s);
        });
}
// The four update `_device` calls: bad argument (njobs < 0 also stands for whatever else the caller refuses at that point), no jobs, missing
// pointers (`have_all`, asked only once there are jobs), then what `prepare` says, then the query -- it knows no pointers: it stages every job,
// decodes every old frame it cannot refuse and counts every record of the stage, so the layout never exceeds it; 0: the limits, taken as the
// query takes them -- then short buffer, then no device; and `launch`.
extern "C++" {
static inline const CbxuBatch &cbu_base(const CbxuBatch &B) { return B; }
template <class BATCH>
static inline const CbxuBatch &cbu_base(const BATCH &B) { return B.U; }      // (the selection and point updates' batches hold the box updates')
template <class BATCH, class HAVE, class PREPARE, class QUERY, class LAUNCH>
static int cbu_device_call(int njobs, int shuffle, int typesize, HAVE have_all, void *d_work, size_t work_bytes, hb_result *d_results, PREPARE prepare, QUERY query,
                           LAUNCH launch) {
    const unsigned policy = hb_cblosc_policy();                           // (hb_cblosc_set_compressor, read once: one call, one policy)
    if (njobs < 0 || typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!have_all() || !d_work || ((uintptr_t)d_work & 255u) || !d_results) return HB_ERR_BAD_ARG;
    uint8_t *w = (uint8_t *)d_work;
    const unsigned accept = hb_cblosc_accepted();                         // (read once: the query below judges the frames as the call does)
    BATCH B;
    const int rc = prepare(B, w, accept);
    if (rc) return rc;
    const size_t q = query(B, accept);
    if (!q) return HB_ERR_BAD_ARG;
    const CbxuBatch &U = cbu_base(B);
    if (work_bytes < q || q < U.L.total || U.X.E.query < U.X.E.L.total) return HB_ERR_SHORT_BUFFER;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    return launch(B, policy, w);
}
}

// ---- many update boxes, one set of launches (include/hipblosc.h; the host side is hb_cblosc_upd_box_batch.h) ----
size_t hb_cblosc_update_boxes_batch_workspace(int njobs, const hb_cblosc_upd_box *boxes, const hb_cblosc_header *old_hdrs, const size_t *old_n, int shuffle, int typesize) {
    return cbxu_workspace(njobs, boxes, old_hdrs, old_n, shuffle, typesize, hb_cblosc_accepted());
}

int hb_cblosc_update_boxes_batch_device(int njobs, const hb_cblosc_upd_box *boxes, const hb_cblosc_header *old_hdrs, const void *const *d_old, const size_t *old_n,
                                        const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize,
                                        void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    return cbu_device_call<CbxuBatch>(
        njobs, shuffle, typesize, [&] { return boxes && old_hdrs && d_old && old_n && d_src && d_frame && cap; }, d_work, work_bytes, d_results,
        [&](CbxuBatch &B, uint8_t *w, unsigned accept) { return cbxu_prepare(njobs, boxes, old_hdrs, d_old, old_n, d_src, d_frame, cap, fill, shuffle, typesize, w, accept, B); },
        [&](const CbxuBatch &, unsigned accept) { return cbxu_workspace(njobs, boxes, old_hdrs, old_n, shuffle, typesize, accept); },
        [&](const CbxuBatch &B, unsigned policy, uint8_t *w) { return cbxu_launch(B, njobs, shuffle, typesize, policy, w, d_results, stream); });
}

// ---- many selection updates, one set of launches (include/hipblosc.h; the host side is hb_cblosc_upd_index_batch.h) ----
size_t hb_cblosc_update_index_batch_workspace(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex, const hb_cblosc_header *old_hdrs,
                                              const size_t *old_n, int shuffle, int typesize) {
    return cbiu_workspace(njobs, jobs, index, nindex, old_hdrs, old_n, shuffle, typesize, hb_cblosc_accepted());
}

int hb_cblosc_update_index_batch_device(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex, const hb_cblosc_header *old_hdrs,
                                        const void *const *d_old, const size_t *old_n, const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill,
                                        int shuffle, int typesize, void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    return cbu_device_call<CbiuBatch>(
        njobs, shuffle, typesize, [&] { return jobs && old_hdrs && d_old && old_n && d_src && d_frame && cap; }, d_work, work_bytes, d_results,
        [&](CbiuBatch &B, uint8_t *w, unsigned accept) {
            return cbiu_prepare(njobs, jobs, index, nindex, old_hdrs, d_old, old_n, d_src, d_frame, cap, fill, shuffle, typesize, w, accept, B);
        },
        [&](const CbiuBatch &, unsigned accept) { return cbiu_workspace(njobs, jobs, index, nindex, old_hdrs, old_n, shuffle, typesize, accept); },
        [&](const CbiuBatch &B, unsigned policy, uint8_t *w) { return cbiu_launch(B, njobs, shuffle, typesize, policy, w, d_results, stream); });
}

// ---- many point updates, one set of launches (include/hipblosc.h; the host side is hb_cblosc_upd_point_batch.h) ----
size_t hb_cblosc_update_points_batch_workspace(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints,
                                               const hb_cblosc_header *old_hdrs, const size_t *old_n, int shuffle, int typesize) {
    return cbpu_workspace(njobs, jobs, points, npoints, old_hdrs, old_n, shuffle, typesize, hb_cblosc_accepted());
}

int hb_cblosc_update_points_batch_device(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints, const hb_cblosc_header *old_hdrs,
                                         const void *const *d_old, const size_t *old_n, const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill,
                                         int shuffle, int typesize, void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    return cbu_device_call<CbpuBatch>(
        njobs, shuffle, typesize, [&] { return jobs && old_hdrs && d_old && old_n && d_src && d_frame && cap; }, d_work, work_bytes, d_results,
        [&](CbpuBatch &B, uint8_t *w, unsigned accept) {
            return cbpu_prepare(njobs, jobs, points, npoints, old_hdrs, d_old, old_n, d_src, d_frame, cap, fill, shuffle, typesize, w, accept, B);
        },
        // (what the sweeps over the points answered is taken from B, not worked out again)
        [&](const CbpuBatch &B, unsigned accept) { return cbpu_workspace(njobs, jobs, points, npoints, old_hdrs, old_n, shuffle, typesize, accept, &B); },
        [&](const CbpuBatch &B, unsigned policy, uint8_t *w) { return cbpu_launch(B, njobs, nullptr, shuffle, typesize, policy, w, d_results, stream); });
}


// ---- prepared point selections (include/hipblosc.h; the host side, the builders and the per-call prepares are hb_cblosc_point_sel.h) ----
}  // extern "C"
struct hb_cblosc_point_sel {
    CbselPlan P;                         // what it keeps on the host: nothing proportional to the points
    CbselKnown W;                        // ... and, derived from it once, what the update's stage takes for its sweeps' answers (per job)
    int device;
    CbpPoint *d_tab;                     // the table of its jobs on `device`: P.npts entries
    bool from_array;                     // built from a mask or coordinates of a whole array:
    std::vector<uint32_t> chunks;        // ... the chunk of every job, in C order of the grid
};
static void cbsel_free(hb_cblosc_point_sel *S) {
    if (S->d_tab) (void)hipFree(S->d_tab);
    delete S;
}
// the selection with its plan begun and its table allocated on the current device
static int cbsel_new(int njobs, const hb_cblosc_sel_job *jobs, int64_t npoints, int typesize, hb_cblosc_point_sel **out) {
    hb_cblosc_point_sel *S = new (std::nothrow) hb_cblosc_point_sel{};
    if (!S) return HB_ERR_BAD_ARG;
    if (hipGetDevice(&S->device) != hipSuccess) { delete S; return HB_ERR_HIP; }
    try { cbsel_begin(njobs, jobs, npoints, typesize, S->P); } catch (const std::bad_alloc &) { delete S; return HB_ERR_BAD_ARG; }
    if (S->P.npts && hipMalloc((void **)&S->d_tab, (size_t)S->P.npts * sizeof(CbpPoint)) != hipSuccess) { S->d_tab = nullptr; delete S; return HB_ERR_HIP; }
    *out = S;
    return HB_OK;
}
// the device builder behind the checks of its callers (the call is not refused as a whole, a device is there, *sel is NULL): the groups of
// jobs through k_cbsel_build, one after the other; synchronises `s`
static int cbsel_create_from_device(int njobs, const hb_cblosc_sel_job *jobs, const hb_cblosc_point *d_points, int64_t npoints, int typesize, hipStream_t s,
                                    hb_cblosc_point_sel **sel) {
    hb_cblosc_point_sel *S = nullptr;
    if (const int rc = cbsel_new(njobs, jobs, npoints, typesize, &S)) return rc;
    uint8_t *d_grp = nullptr;
    size_t grp_bytes = 0;
    int rc = HB_OK;
    try {
        CbselGroup G;
        std::vector<uint8_t> up, down;
        for (size_t from = 0, nj = S->P.jobs.size(); from < nj && rc == HB_OK;) {
            from = cbsel_next_group(S->P, from, G);
            const size_t ng = G.rec.size();
            if (!ng) break;
            const CbselGroupLayout &L = G.L;
            if (L.total > grp_bytes) {                                    // (the groups' memory is the builder's own, freed before it returns)
                if (d_grp) (void)hipFree(d_grp);
                d_grp = nullptr; grp_bytes = 0;
                if (hipMalloc((void **)&d_grp, L.total) != hipSuccess) { d_grp = nullptr; rc = HB_ERR_HIP; break; }
                grp_bytes = L.total;
            }
            // the words and both bitmaps are cleared; the records and their prefix go up in one copy (the buffer is read before the call returns)
            up.assign(L.out, 0);
            memcpy(up.data() + L.jobs, G.rec.data(), ng * sizeof(CbselJob));
            memcpy(up.data() + L.blk, G.blk.data(), (ng + 1) * 4);
            if (hipMemsetAsync(d_grp + L.out, 0, L.total - L.out, s) != hipSuccess || hipMemcpyAsync(d_grp, up.data(), L.out, hipMemcpyHostToDevice, s) != hipSuccess) { rc = HB_ERR_HIP; break; }
            hb_prof_begin("k_cbsel_build", s);
            hipLaunchKernelGGL(k_cbsel_build, dim3(G.blk.back()), dim3(256), 0, s, (const CbselJob *)(d_grp + L.jobs), (const uint32_t *)(d_grp + L.blk), (uint32_t)ng, d_points,
                               S->d_tab, (uint32_t)typesize, ~0ull / (uint64_t)typesize, (uint32_t *)(d_grp + L.ibits), (uint32_t *)(d_grp + L.bbits), (CbselOut *)(d_grp + L.out));
            hb_prof_end(s);
            // the per-job words and the block bitmaps come down in one copy; the item bitmaps stay where they are
            down.resize(L.ibits - L.out);
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(down.data(), d_grp + L.out, down.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess) { rc = HB_ERR_HIP; break; }
            cbsel_take_group(S->P, G, (const CbselOut *)down.data(), (const uint32_t *)(down.data() + (L.bbits - L.out)));
        }
        if (rc == HB_OK && hipStreamSynchronize(s) != hipSuccess) rc = HB_ERR_HIP;
        if (rc == HB_OK) cbsel_known(S->P, S->W);
    } catch (const std::bad_alloc &) { (void)hipStreamSynchronize(s); rc = HB_ERR_BAD_ARG; }
    if (d_grp) (void)hipFree(d_grp);
    if (rc) { cbsel_free(S); return rc; }
    *sel = S;
    return HB_OK;
}

// ---- selections from device masks and coordinate arrays (include/hipblosc.h; hb_cblosc_array_sel.h) ----
// the builder's own device memory: one allocation of sections, each 256-byte aligned, and the temporary points
struct CbasMem {
    uint8_t *d_work = nullptr;
    hb_cblosc_point *d_pts = nullptr;
    ~CbasMem() { if (d_work) (void)hipFree(d_work); if (d_pts) (void)hipFree(d_pts); }
};
// exclusive prefix sums of the n words at `counts` into out0 (and, in array order, out1 where orders == 2; else out1 is not looked at): n + 1 words each
static void cbas_scan_launch(const CbasGeom &g, const uint32_t *counts, uint32_t n, uint32_t orders, uint32_t *tile_sum, uint32_t *tile_pre, uint32_t *out0, uint32_t *out1, hipStream_t s) {
    const uint32_t ntiles = cbas_ntiles(n);
    hb_prof_begin("k_cbas_tiles", s);
    hipLaunchKernelGGL(k_cbas_tiles, dim3(ntiles, orders), dim3(256), 0, s, g, counts, n, ntiles, tile_sum);
    hb_prof_end(s);
    hb_prof_begin("k_cbas_scan", s);
    hipLaunchKernelGGL(k_cbas_scan, dim3(orders), dim3(256), 0, s, (const uint32_t *)tile_sum, tile_pre, ntiles);
    hb_prof_end(s);
    hb_prof_begin("k_cbas_apply", s);
    hipLaunchKernelGGL(k_cbas_apply, dim3(ntiles, orders), dim3(256), 0, s, g, counts, n, ntiles, (const uint32_t *)tile_pre, out0, out1);
    hb_prof_end(s);
}
// the jobs of the chunks with points over the temporary points -> the selection, which remembers its chunks
static int cbas_finish(const std::vector<hb_cblosc_sel_job> &jobs, std::vector<uint32_t> &chunks, const hb_cblosc_point *d_pts, int64_t npoints, int typesize, hipStream_t s,
                       hb_cblosc_point_sel **sel) {
    if (jobs.size() > (size_t)0x7FFFFFFF) return HB_ERR_BAD_ARG;
    const int rc = cbsel_create_from_device((int)jobs.size(), jobs.data(), d_pts, npoints, typesize, s, sel);
    if (rc) return rc;
    (*sel)->from_array = true;
    (*sel)->chunks.swap(chunks);
    return HB_OK;
}
static int cbas_create_mask(const CbasGeom &g, int64_t chunk_items, uint32_t blocksize, const uint8_t *d_mask, int typesize, hipStream_t s, hb_cblosc_point_sel **sel) {
    CbasMem M;
    const uint32_t nrows = g.nrows, ntiles = cbas_ntiles(nrows);
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += cb_align(b); return at; };
    const size_t o_counts = take((size_t)nrows * 4), o_cm = take(((size_t)nrows + 1) * 4), o_ar = take(((size_t)nrows + 1) * 4), o_tsum = take((size_t)ntiles * 8),
                 o_tpre = take((size_t)ntiles * 8), o_pairs = take((size_t)g.nchunks * 8);
    if (hipMalloc((void **)&M.d_work, o) != hipSuccess) { M.d_work = nullptr; return HB_ERR_HIP; }
    uint8_t *w = M.d_work;
    uint32_t *counts = (uint32_t *)(w + o_counts), *scan_cm = (uint32_t *)(w + o_cm), *scan_ar = (uint32_t *)(w + o_ar), *pairs = (uint32_t *)(w + o_pairs);
    const uint32_t row_groups = (uint32_t)(((uint64_t)nrows + CBAS_ROWS_PER_GROUP - 1u) / CBAS_ROWS_PER_GROUP);
    hb_prof_begin("k_cbas_mask_count", s);
    hipLaunchKernelGGL(k_cbas_mask_count, dim3(row_groups), dim3(256), 0, s, g, d_mask, counts);
    hb_prof_end(s);
    cbas_scan_launch(g, counts, nrows, 2u, (uint32_t *)(w + o_tsum), (uint32_t *)(w + o_tpre), scan_cm, scan_ar, s);
    hb_prof_begin("k_cbas_chunks", s);
    hipLaunchKernelGGL(k_cbas_chunks, dim3((g.nchunks + 255u) / 256u), dim3(256), 0, s, g, (const uint32_t *)scan_cm, pairs);
    hb_prof_end(s);
    // the per-chunk records come down: the one download that grows with the grid
    std::vector<uint32_t> down((size_t)g.nchunks * 2);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(down.data(), pairs, down.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return HB_ERR_HIP;
    std::vector<hb_cblosc_sel_job> jobs;
    std::vector<uint32_t> chunks;
    cbas_jobs(g.nchunks, down.data(), down.data() + 1, 2, chunk_items, blocksize, jobs, chunks);
    const uint64_t npts = jobs.empty() ? 0u : (uint64_t)jobs.back().first + (uint64_t)jobs.back().count;
    if (npts > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
    if (npts) {
        if (hipMalloc((void **)&M.d_pts, (size_t)npts * sizeof(hb_cblosc_point)) != hipSuccess) { M.d_pts = nullptr; return HB_ERR_HIP; }
        hb_prof_begin("k_cbas_mask_emit", s);
        hipLaunchKernelGGL(k_cbas_mask_emit, dim3(row_groups), dim3(256), 0, s, g, d_mask, (const uint32_t *)scan_cm, (const uint32_t *)scan_ar, M.d_pts);
        hb_prof_end(s);
        if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return HB_ERR_HIP; }
    }
    return cbas_finish(jobs, chunks, M.d_pts, (int64_t)npts, typesize, s, sel);      // (it synchronises `s`: the temporary memory may go)
}
static int cbas_create_coords(const CbasGeom &g, int64_t chunk_items, uint32_t blocksize, const int64_t *const *d_coords, int ndim, uint32_t npoints, int typesize, hipStream_t s,
                              hb_cblosc_point_sel **sel) {
    CbasMem M;
    const uint32_t nchunks = g.nchunks, ntiles = cbas_ntiles(nchunks);
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += cb_align(b); return at; };
    // [counters | their prefix, n + 1 words | the flag word] lie together: they come down in one copy
    const size_t o_cnt = 0, o_first = (size_t)nchunks * 4, o_flag = o_first + ((size_t)nchunks + 1) * 4, head = o_flag + 4;
    take(head);
    const size_t o_tsum = take((size_t)ntiles * 4), o_tpre = take((size_t)ntiles * 4), o_rec = take((size_t)npoints * sizeof(CbasRec));
    if (hipMalloc((void **)&M.d_work, o) != hipSuccess) { M.d_work = nullptr; return HB_ERR_HIP; }
    if (hipMalloc((void **)&M.d_pts, (size_t)npoints * sizeof(hb_cblosc_point)) != hipSuccess) { M.d_pts = nullptr; return HB_ERR_HIP; }
    uint8_t *w = M.d_work;
    uint32_t *counters = (uint32_t *)(w + o_cnt), *first = (uint32_t *)(w + o_first), *flag = (uint32_t *)(w + o_flag);
    CbasRec *rec = (CbasRec *)(w + o_rec);
    CbasCoords X{};
    for (int k = 0; k < ndim; k++) X.p[(4 - ndim) + k] = d_coords[k];
    if (hipMemsetAsync(w, 0, head, s) != hipSuccess) return HB_ERR_HIP;
    const uint32_t groups = (uint32_t)(((uint64_t)npoints + 255u) / 256u);
    hb_prof_begin("k_cbas_coord_bucket", s);
    hipLaunchKernelGGL(k_cbas_coord_bucket, dim3(groups), dim3(256), 0, s, g, X, npoints, counters, flag, rec);
    hb_prof_end(s);
    cbas_scan_launch(g, counters, nchunks, 1u, (uint32_t *)(w + o_tsum), (uint32_t *)(w + o_tpre), first, nullptr, s);
    std::vector<uint32_t> down(head / 4);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(down.data(), w, head, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return HB_ERR_HIP;
    if (down[o_flag / 4]) return HB_ERR_BAD_ARG;                          // a coordinate outside the array
    hb_prof_begin("k_cbas_coord_place", s);
    hipLaunchKernelGGL(k_cbas_coord_place, dim3(groups), dim3(256), 0, s, (const CbasRec *)rec, (const uint32_t *)first, M.d_pts, npoints);
    hb_prof_end(s);
    if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return HB_ERR_HIP; }
    std::vector<hb_cblosc_sel_job> jobs;
    std::vector<uint32_t> chunks;
    cbas_jobs(nchunks, down.data() + o_first / 4, down.data() + o_cnt / 4, 1, chunk_items, blocksize, jobs, chunks);
    return cbas_finish(jobs, chunks, M.d_pts, (int64_t)npoints, typesize, s, sel);
}
// a selection of no jobs (an empty array, no points)
static int cbas_create_empty(int typesize, hipStream_t s, hb_cblosc_point_sel **sel) {
    std::vector<hb_cblosc_sel_job> jobs;
    std::vector<uint32_t> chunks;
    return cbas_finish(jobs, chunks, nullptr, 0, typesize, s, sel);
}
extern "C" {
int hb_cblosc_point_sel_create(int njobs, const hb_cblosc_sel_job *jobs, const hb_cblosc_point *points, int64_t npoints, int typesize, int device,
                               hb_cblosc_point_sel **sel) {
    if (sel) *sel = nullptr;
    if (cbsel_call_refused(njobs, jobs, points, npoints, typesize, sel)) return HB_ERR_BAD_ARG;
    if (const int rc = hb_select_device(device)) return rc;
    hb_cblosc_point_sel *S = nullptr;
    if (const int rc = cbsel_new(njobs, jobs, npoints, typesize, &S)) return rc;
    try {
        std::vector<CbpPoint> tab;
        cbsel_build_host(S->P, points, tab);
        cbsel_known(S->P, S->W);
        if (!tab.empty() && hipMemcpy(S->d_tab, tab.data(), tab.size() * sizeof(CbpPoint), hipMemcpyHostToDevice) != hipSuccess) { cbsel_free(S); return HB_ERR_HIP; }
    } catch (const std::bad_alloc &) { cbsel_free(S); return HB_ERR_BAD_ARG; }
    *sel = S;
    return HB_OK;
}

int hb_cblosc_point_sel_create_device(int njobs, const hb_cblosc_sel_job *jobs, const hb_cblosc_point *d_points, int64_t npoints, int typesize, void *stream,
                                      hb_cblosc_point_sel **sel) {
    if (sel) *sel = nullptr;
    if (cbsel_call_refused(njobs, jobs, d_points, npoints, typesize, sel) || ((uintptr_t)d_points & 15u)) return HB_ERR_BAD_ARG;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    return cbsel_create_from_device(njobs, jobs, d_points, npoints, typesize, (hipStream_t)stream, sel);
}

int hb_cblosc_point_sel_create_mask_device(const hb_cblosc_sel_array *a, const void *d_mask, int typesize, void *stream, hb_cblosc_point_sel **sel) {
    if (sel) *sel = nullptr;
    CbasGeom g;
    int64_t chunk_items;
    bool empty;
    const int refused = cbas_refusal(a, typesize, 0, sel, g, chunk_items, empty);
    if (refused == HB_ERR_BAD_ARG || (!empty && !d_mask)) return HB_ERR_BAD_ARG;      // (every HB_ERR_BAD_ARG comes before HB_ERR_DATA_TOO_LARGE)
    if (refused) return refused;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    try {
        if (empty) return cbas_create_empty(typesize, (hipStream_t)stream, sel);
        return cbas_create_mask(g, chunk_items, a->blocksize, (const uint8_t *)d_mask, typesize, (hipStream_t)stream, sel);
    } catch (const std::bad_alloc &) { (void)hipStreamSynchronize((hipStream_t)stream); return HB_ERR_BAD_ARG; }
}

int hb_cblosc_point_sel_create_coords_device(const hb_cblosc_sel_array *a, const int64_t *const *d_coords, int64_t npoints, int typesize, void *stream,
                                             hb_cblosc_point_sel **sel) {
    if (sel) *sel = nullptr;
    CbasGeom g;
    int64_t chunk_items;
    bool empty;
    const int refused = cbas_refusal(a, typesize, npoints, sel, g, chunk_items, empty);
    if (refused == HB_ERR_BAD_ARG || cbas_coords_refused(a, d_coords, npoints)) return HB_ERR_BAD_ARG;
    if (refused) return refused;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    try {
        if (npoints == 0) return cbas_create_empty(typesize, (hipStream_t)stream, sel);
        if (empty) return HB_ERR_BAD_ARG;                                 // (a point of an array without items lies outside it)
        return cbas_create_coords(g, chunk_items, a->blocksize, d_coords, a->ndim, (uint32_t)npoints, typesize, (hipStream_t)stream, sel);
    } catch (const std::bad_alloc &) { (void)hipStreamSynchronize((hipStream_t)stream); return HB_ERR_BAD_ARG; }
}

int hb_cblosc_point_sel_njobs(const hb_cblosc_point_sel *sel) { return sel ? (int)sel->P.jobs.size() : HB_ERR_BAD_ARG; }
int64_t hb_cblosc_point_sel_npoints(const hb_cblosc_point_sel *sel) { return sel ? (int64_t)sel->P.npts : (int64_t)HB_ERR_BAD_ARG; }
int hb_cblosc_point_sel_job_chunks(const hb_cblosc_point_sel *sel, uint32_t *chunk, int n) {
    if (!sel || !chunk || !sel->from_array || n < 0 || (size_t)n != sel->P.jobs.size()) return HB_ERR_BAD_ARG;
    for (size_t j = 0; j < sel->chunks.size(); j++) chunk[j] = sel->chunks[j];
    return HB_OK;
}
// the job's table entries come down as they lie and become {item, out} again (an entry holds both times the typesize)
int hb_cblosc_point_sel_job_points(const hb_cblosc_point_sel *sel, int job, hb_cblosc_point *points, int64_t n) {
    if (!sel || job < 0 || (size_t)job >= sel->P.jobs.size()) return HB_ERR_BAD_ARG;
    const CbselEntry &E = sel->P.jobs[(size_t)job];
    if (E.status || n != E.count || (n > 0 && !points)) return HB_ERR_BAD_ARG;
    if (n == 0) return HB_OK;
    const int dev = sel->device;
    int cur = -1, rc = HB_OK;
    if (hipGetDevice(&cur) != hipSuccess || (cur != dev && hipSetDevice(dev) != hipSuccess)) return HB_ERR_HIP;
    static_assert(sizeof(hb_cblosc_point) == sizeof(CbpPoint), "the entries come down into the caller's points");
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(points, sel->d_tab + E.pt0, (size_t)n * sizeof(CbpPoint), hipMemcpyDeviceToHost) != hipSuccess) rc = HB_ERR_HIP;
    if (cur != dev) (void)hipSetDevice(cur);
    if (rc) return rc;
    const uint64_t ts = (uint64_t)sel->P.typesize;
    for (int64_t p = 0; p < n; p++) {
        CbpPoint e;
        memcpy(&e, points + p, sizeof e);
        points[p] = hb_cblosc_point{(int64_t)(e.off / ts), (int64_t)(e.out / ts)};
    }
    return HB_OK;
}

int hb_cblosc_point_sel_destroy(hb_cblosc_point_sel *sel) {
    if (!sel) return HB_OK;
    const int dev = sel->device;
    int cur = -1, rc = HB_OK;
    // (work enqueued with the selection may still read its table: the device is drained before the table goes)
    if (hipGetDevice(&cur) != hipSuccess || (cur != dev && hipSetDevice(dev) != hipSuccess) || hipDeviceSynchronize() != hipSuccess) rc = HB_ERR_HIP;
    cbsel_free(sel);
    if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
    return rc;
}

int hb_cblosc_point_sel_info(const hb_cblosc_point_sel *sel, int job, hb_cblosc_sel_info *info) {
    if (!sel || !info || job < 0 || (size_t)job >= sel->P.jobs.size()) return HB_ERR_BAD_ARG;
    cbsel_info(sel->P.jobs[(size_t)job], *info);
    return HB_OK;
}

size_t hb_cblosc_point_sel_device_bytes(const hb_cblosc_point_sel *sel) { return sel ? (size_t)sel->P.npts * sizeof(CbpPoint) : 0; }

// whether the current device is the selection's
static bool cbsel_on_device(const hb_cblosc_point_sel *sel) {
    int cur = -1;
    return hipGetDevice(&cur) == hipSuccess && cur == sel->device;
}

size_t hb_cblosc_getpoints_sel_workspace(const hb_cblosc_point_sel *sel, int nframes, const hb_cblosc_header *hdrs, const size_t *n, const uint32_t *job_frame) {
    if (!sel) return 0;
    return cbsel_read_workspace(sel->P, nframes, hdrs, n, job_frame, hb_cblosc_accepted());
}

int hb_cblosc_getpoints_sel_device(const hb_cblosc_point_sel *sel, int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n,
                                   const uint32_t *job_frame, void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    if (!sel || !job_frame) return HB_ERR_BAD_ARG;
    const int njobs = (int)sel->P.jobs.size();
    const int rc = cbx_device_call(
        nframes, njobs, hdrs && d_frame && n && d_dst && cap && cbsel_on_device(sel), d_work, work_bytes, d_results, stream,
        [&](CbxBatch &B, unsigned accept) { return cbsel_read_prepare(sel->P, nframes, hdrs, d_frame, n, job_frame, d_dst, cap, true, B, accept); },
        [&](unsigned accept) { return cbsel_read_workspace(sel->P, nframes, hdrs, n, job_frame, accept); }, sel->d_tab);
    return rc;
}

size_t hb_cblosc_update_points_sel_workspace(const hb_cblosc_point_sel *sel, const hb_cblosc_header *old_hdrs, const size_t *old_n, int shuffle, int typesize) {
    if (!sel) return 0;
    CbpuBatch B;
    if (cbsel_update_prepare(sel->P, sel->W, old_hdrs, nullptr, old_n, nullptr, nullptr, nullptr, nullptr, shuffle, typesize, nullptr, hb_cblosc_accepted(), B)) return 0;
    return B.query;
}

int hb_cblosc_update_points_sel_device(const hb_cblosc_point_sel *sel, const hb_cblosc_header *old_hdrs, const void *const *d_old, const size_t *old_n,
                                       const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize,
                                       void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    const int njobs = sel && typesize == sel->P.typesize ? (int)sel->P.jobs.size() : -1;      // (-1: refused with the bad arguments)
    return cbu_device_call<CbpuBatch>(
        njobs, shuffle, typesize, [&] { return old_hdrs && d_old && old_n && d_src && d_frame && cap && cbsel_on_device(sel); }, d_work, work_bytes, d_results,
        [&](CbpuBatch &B, uint8_t *w, unsigned accept) {
            return cbsel_update_prepare(sel->P, sel->W, old_hdrs, d_old, old_n, d_src, d_frame, cap, fill, shuffle, typesize, w, accept, B);
        },
        [&](const CbpuBatch &, unsigned accept) {                         // (a second prepare, without pointers)
            CbpuBatch Q;
            return cbsel_update_prepare(sel->P, sel->W, old_hdrs, nullptr, old_n, nullptr, nullptr, nullptr, nullptr, shuffle, typesize, nullptr, accept, Q) ? (size_t)0 : Q.query;
        },
        [&](const CbpuBatch &B, unsigned policy, uint8_t *w) { return cbpu_launch(B, njobs, sel->d_tab, shuffle, typesize, policy, w, d_results, stream); });
}
}  // extern "C"
