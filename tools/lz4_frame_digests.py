#!/usr/bin/env python3
"""tools/lz4_frame_digests.py --commit ID [--out tests/golden/lz4_frame_digests.json]: SHA-256 of the LZ4 frames that the library in use
(HIPBLOSC_LIB selects another build of it) writes on the GPU for the inputs of tests/lz4_diet_cases.py, with and without the index
trailer.  Run with the library of the commit named by --commit BEFORE a change to the LZ4 kernels; tests/test_gpu_lz4_diet.py then holds
every later encoder to these bytes."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lz4_frame_digests.json"))
    a = ap.parse_args()
    import hipblosc as hb
    import oracle as O
    import devmem as D
    import lz4_diet_cases as C
    O.build()
    assert hb.lib().hb_init() == 0, "no HIP device"
    inputs, frames = {}, {}
    for name, x, s, ts, lv in C.cases(O):
        inputs[name.split("-")[0]] = C.digest(x)
        t = C.compress(hb, D, x, s, ts, lv, hb.OPT_INDEX_TRAILER)
        p = C.compress(hb, D, x, s, ts, lv, 0)
        frames[name] = {"n": int(x.size), "trailer": C.digest(t), "trailer_bytes": len(t), "plain": C.digest(p), "plain_bytes": len(p), "flags": t[2]}
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "library": os.path.basename(hb.LIB_PATH), "inputs": inputs, "frames": frames}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(frames)} cases -> {a.out}")


if __name__ == "__main__":
    main()
