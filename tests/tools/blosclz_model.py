"""BloscLZ streams of C-Blosc-1 frames in pure Python: the specification the device decoder is checked against, and the means to build
exact edge cases by hand (tests/test_cblosc_blosclz_cpu.py checks all of it against c-blosc 1.21 / BloscLZ 2.3.0 used as a black box;
tests/test_gpu_cblosc_blosclz.py checks the device against it and the library).

  decode(stream, usize)          the stream decoder, bounds-checked: the bytes, or None where blosclz_decompress refuses
  parse(stream)                  the elements of a stream and its statistics (no output is built)
  frame_streams(frame)           every stream of a frame with its sizes and element statistics
  decode_frame(frame)            all streams decoded, filters NOT undone (equals the input for an unfiltered frame); None on any failure
  build_stream(elements)         [("lit", bytes) | ("match", dist, len)] -> stream bytes
  build_frame(blocks, ...)       header, bstarts, { int32 size, bytes } per stream

The format.  A control byte c; the stream's first one counts with its three high bits cleared, so it is always a literal run.
  c < 32   c + 1 literal bytes follow
  c >= 32  a match: length (c >> 5) - 1, and when that is 6 the bytes that follow are added up to and including the first that is not
           255; then 3 more.  Distance ((c & 31) << 8) + next byte + 1 -- unless that byte is 255 and c & 31 is 31: then two more
           bytes, big-endian, + 8192 (8192 .. 73727: more than 16 bits).  Distance 1 is a run of the previous byte; copies go byte
           by byte, an overlap repeats.
The decoder reads the next control byte BEFORE it copies a match, and stops -- without the copy -- when the input is used up there: a
stream that ends in a match comes out short, which the frame layer refuses.  It also asks for one more byte than it reads at every
byte of a match header (`ip + 1 >= ip_limit`), which comes to the same thing: a match is never the last element.
"""
import struct

MAX_NEAR = 8191            # the largest distance of the short form
MAX_DIST = 65535 + 8192    # ... of the long one
MAX_LIT = 32


def _walk(src, usize, out):
    """The decoder's loop.  out: a bytearray to fill, or None (statistics only).  Returns (produced or None, stats)."""
    st = {"elements": 0, "matches": 0, "max_dist": 0, "far": 0, "chain": 0, "max_len": 0}
    n = len(src)
    if n == 0:
        return 0, st
    ip, op = 1, 0
    c = src[0] & 31
    while True:
        st["elements"] += 1
        if c >= 32:
            ln = (c >> 5) - 1
            ofs = (c & 31) << 8
            chain = 0
            if ln == 6:
                while True:
                    if ip + 1 >= n:
                        return None, st
                    code = src[ip]; ip += 1
                    ln += code; chain += 1
                    if code != 255:
                        break
            elif ip + 1 >= n:
                return None, st
            code = src[ip]; ip += 1
            ln += 3
            dist = ofs + code
            far = code == 255 and ofs == 31 << 8
            if far:
                if ip + 1 >= n:
                    return None, st
                dist = (src[ip] << 8) + src[ip + 1] + MAX_NEAR
                ip += 2
            dist += 1
            if op + ln > usize or dist > op:
                return None, st
            st["matches"] += 1; st["far"] += far
            st["max_dist"] = max(st["max_dist"], dist); st["chain"] = max(st["chain"], chain); st["max_len"] = max(st["max_len"], ln)
            if ip >= n:
                break                                   # the stream ends in a match: NOT copied
            c = src[ip]; ip += 1
            if out is not None:
                if dist >= ln:
                    out[op:op + ln] = out[op - dist:op - dist + ln]
                else:
                    pat = bytes(out[op - dist:op])
                    out[op:op + ln] = (pat * (ln // dist + 1))[:ln]
            op += ln
        else:
            ln = c + 1
            if op + ln > usize or ip + ln > n:
                return None, st
            if out is not None:
                out[op:op + ln] = src[ip:ip + ln]
            op += ln; ip += ln
            if ip >= n:
                break
            c = src[ip]; ip += 1
    return op, st


def decode(stream, usize):
    """The `usize` bytes a compressed stream decodes to, or None: a stream the library refuses, or one that does not produce exactly usize."""
    out = bytearray(usize)
    got, _ = _walk(bytes(stream), usize, out)
    return bytes(out) if got == usize else None


def parse(stream, usize=1 << 31):
    """(ok, stats) of a compressed stream: elements, matches, max_dist, far (matches in the long form), chain (most added length bytes), max_len."""
    got, st = _walk(bytes(stream), usize, None)
    return got is not None, st


def nsplit_of(flags, typesize, blocksize):
    return typesize if not flags & 0x10 and 1 <= typesize <= 16 and blocksize // typesize >= 128 else 1


def frame_streams(frame):
    """Every stream of a C-Blosc-1 frame that is not memcpyed: dicts with block, index, src (offset of the bytes), csize, usize, dst (offset in
    the decoded, still filtered frame), stored, and -- for a compressed stream -- ok and the statistics of parse().  Raises ValueError on a
    frame whose tables do not hold."""
    ver, verlz, flags, ts, nbytes, bs, cbytes = struct.unpack("<BBBBIII", frame[:16])
    if flags & 0x02 or nbytes == 0:
        return
    nblocks = (nbytes + bs - 1) // bs
    for b in range(nblocks):
        bsize = min(bs, nbytes - b * bs)
        ns = nsplit_of(flags, ts, bs) if bsize == bs else 1
        p, = struct.unpack_from("<I", frame, 16 + 4 * b)
        ne = bsize // ns
        for s in range(ns):
            if p + 4 > len(frame):
                raise ValueError("stream header beyond the frame")
            cs, = struct.unpack_from("<i", frame, p)
            p += 4
            if cs <= 0 or p + cs > len(frame):
                raise ValueError("stream beyond the frame")
            rec = {"block": b, "index": s, "src": p, "csize": cs, "usize": ne, "dst": b * bs + s * ne, "stored": cs == ne}
            if not rec["stored"]:
                ok, st = parse(frame[p:p + cs], ne)
                rec["ok"] = ok
                rec.update(st)
            yield rec
            p += cs


def decode_frame(frame):
    """The decoded bytes of all streams in place, filters not undone; None when a stream fails.  A memcpyed frame: its bytes."""
    ver, verlz, flags, ts, nbytes, bs, cbytes = struct.unpack("<BBBBIII", frame[:16])
    if flags & 0x02:
        return bytes(frame[16:16 + nbytes])
    out = bytearray(nbytes)
    try:
        for r in frame_streams(frame):
            raw = frame[r["src"]:r["src"] + r["csize"]]
            d = bytes(raw) if r["stored"] else decode(raw, r["usize"])
            if d is None:
                return None
            out[r["dst"]:r["dst"] + r["usize"]] = d
    except (ValueError, struct.error):
        return None
    return bytes(out)


def build_stream(elements, first_high_bits=0):
    """[("lit", bytes) | ("match", dist, len)] -> stream bytes.  A literal run of more than 32 bytes becomes several; a match has len >= 3 and
    1 <= dist <= 73727 (from 8192 on in the long form).  first_high_bits: OR-ed into the first control byte (0x20 .. 0xE0), which the decoder
    must ignore there."""
    out = bytearray()
    for e in elements:
        if e[0] == "lit":
            data = bytes(e[1])
            assert data
            for i in range(0, len(data), MAX_LIT):
                part = data[i:i + MAX_LIT]
                out.append(len(part) - 1)
                out += part
        else:
            _, dist, ln = e
            assert ln >= 3 and 1 <= dist <= MAX_DIST and out, e
            v = ln - 3
            d = dist - 1
            lo = 31 if d >= MAX_NEAR else d >> 8
            if v < 6:
                out.append(((v + 1) << 5) | lo)
            else:
                out.append((7 << 5) | lo)
                v -= 6
                while v >= 255:
                    out.append(255); v -= 255
                out.append(v)
            if d >= MAX_NEAR:
                d -= MAX_NEAR
                out += bytes([255, d >> 8, d & 255])
            else:
                out.append(d & 255)
    assert out and out[0] < 32, "a stream begins with a literal run"
    out[0] |= first_high_bits
    return bytes(out)


def expand(elements):
    """What the elements decode to (the builder's own arithmetic, independent of decode())."""
    out = bytearray()
    for e in elements:
        if e[0] == "lit":
            out += e[1]
        else:
            _, dist, ln = e
            assert dist <= len(out)
            for _ in range(ln):
                out.append(out[-dist])
    return bytes(out)


def build_frame(blocks, nbytes, blocksize, typesize=1, flags=0x10, version=2, versionlz=1):
    """blocks: per block the list of its streams' bytes as they lie in the frame (compressed, or stored = exactly the stream's size).
    flags: 0x10 not split, 0x01 / 0x04 the filters; the codec format bits stay 0 (BloscLZ) unless given."""
    nblocks = len(blocks)
    assert nblocks == (nbytes + blocksize - 1) // blocksize
    body, bstarts = bytearray(), []
    at = 16 + 4 * nblocks
    for streams in blocks:
        bstarts.append(at + len(body))
        for s in streams:
            body += struct.pack("<i", len(s)) + bytes(s)
    head = bytes([version, versionlz, flags, typesize]) + struct.pack("<III", nbytes, blocksize, at + len(body))
    return head + b"".join(struct.pack("<I", x) for x in bstarts) + bytes(body)
