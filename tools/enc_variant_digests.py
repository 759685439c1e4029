#!/usr/bin/env python3
"""tools/enc_variant_digests.py --commit ID [--out tests/golden/enc_variant_digests.json]: SHA-256 of what the library in use (HIPBLOSC_LIB
selects another build of it) writes on the GPU for the inputs of tests/enc_variant_cases.py -- the instantiations of the matcher that
tests/golden/lz4_frame_digests.json does not pin: LZ4HC at 1 / 2 / 4 candidates per bucket, Snappy, the self-contained matchers of the
C-Blosc-1 writers under every policy, the inputs of the batch encoder, the lengths at which the step loop's head / INNER / tail bodies
hand over.  Run with the library of the commit named by --commit BEFORE a change to the matcher; tests/test_gpu_enc_variants.py then
holds every later encoder to these bytes.  A memcpy frame (header flag 0x2) pins nothing of the emitter: the tool refuses to write a
JSON that holds one."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("go-blosc_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library wrote the frames")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "enc_variant_digests.json"))
    a = ap.parse_args()
    import hipblosc as hb
    import oracle as O
    import devmem as D
    import lz4_diet_cases as C
    import enc_variant_cases as V
    O.build()
    assert hb.lib().hb_init() == 0, "no HIP device"
    inputs, frames, cblosc, memcpyed = {}, {}, {}, []
    for name, x, codec, level, shuffle, ts in V.frame_cases():
        inputs[name] = C.digest(x)
        row = {"n": int(x.size)}
        for kind, opts in V.opts_of(hb, codec):
            f = V.compress(hb, D, x, codec, level, shuffle, ts, opts)
            row[kind], row[kind + "_bytes"], row["flags"] = C.digest(f), len(f), f[2]
            if f[2] & hb.flagMemcpy:
                memcpyed.append(f"{name} ({kind})")
        frames[name] = row
    for name, x, codec, clevel, ts in V.cblosc_cases(O):
        inputs[name] = C.digest(x)
        f = V.cblosc_compress(hb, D, x, codec, clevel, ts)
        cblosc[name] = {"n": int(x.size), "frame": C.digest(f), "frame_bytes": len(f), "flags": f[2]}
        if f[2] & 0x02:                                   # BLOSC_MEMCPYED
            memcpyed.append(name)
    if memcpyed:
        raise SystemExit("memcpy frames pin nothing of the emitter; choose other inputs for: " + ", ".join(memcpyed))
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "library": os.path.basename(hb.LIB_PATH), "inputs": inputs, "frames": frames, "cblosc": cblosc}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(frames)} frame cases, {len(cblosc)} C-Blosc-1 cases -> {a.out}")


if __name__ == "__main__":
    main()
