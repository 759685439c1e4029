"""Device memory for tests of the `_dev` entry points: one hipMalloc arena per test, every buffer in it behind guard zones.

The host-pointer entry points stage through pool buffers with slack behind every input and output, so a kernel that writes past
its buffer, or reads scratch it never wrote, passes through them unseen.  Here every buffer has a seeded pattern in front of and
behind it (check_guards() names the buffer and the first changed byte), outputs get exactly the capacity the call is given, and
sources get exactly the 16 bytes of slack include/hipblosc.h allows (read, never written: checked like a guard).

Device memory goes through libamdhip64.so, the runtime libhipblosc.so itself is linked to: a second runtime in the process (torch's)
would not see the GPU (test_gpu_foreign.py).  layout() is pure arithmetic, checked on the CPU (test_abi.py).
"""
import ctypes
from dataclasses import dataclass

import numpy as np

GUARD = 4096          # bytes of pattern in front of every buffer and behind every output / workspace
SRC_TAIL = 16         # behind a source: a `_dev` source may be read up to 15 bytes past its end, never written (include/hipblosc.h)
H2D, D2H = 1, 2


@dataclass(frozen=True)
class Slot:
    name: str
    off: int          # first byte of the buffer, from the arena base
    nbytes: int
    lo: int           # front guard: [lo, off)
    hi: int           # back guard: [off + nbytes, hi)
    source: bool


def layout(specs, guard=GUARD):
    """specs: (name, nbytes, misalign, source) -> ([Slot], arena bytes).  A buffer starts at `misalign` past a 256-byte boundary (the
    arena base is one), with at least `guard` bytes of front guard; outputs and workspaces get `guard` bytes behind them, sources exactly
    SRC_TAIL.  Sources come last, so the last one ends SRC_TAIL bytes before the end of the allocation."""
    slots, o = [], 0
    for name, nbytes, mis, source in sorted(specs, key=lambda s: bool(s[3])):
        assert 0 <= mis < 256 and nbytes >= 0
        off = (o + guard + 255) // 256 * 256 + mis
        hi = off + nbytes + (SRC_TAIL if source else guard)
        slots.append(Slot(name, off, nbytes, o, hi, bool(source)))
        o = hi
    return slots, o


def out(name, nbytes, mis=0):
    return (name, int(nbytes), mis, False)


def src(name, nbytes, mis=0):
    return (name, int(nbytes), mis, True)


_hip = None


def hip():
    global _hip
    if _hip is None:
        h = ctypes.CDLL("libamdhip64.so")
        vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        for name, args in (("hipMalloc", [ctypes.POINTER(vp), sz]), ("hipFree", [vp]), ("hipMemcpy", [vp, vp, sz, i32]),
                           ("hipMemset", [vp, i32, sz]), ("hipDeviceSynchronize", []), ("hipStreamCreate", [ctypes.POINTER(vp)]),
                           ("hipStreamDestroy", [vp]), ("hipStreamSynchronize", [vp])):
            getattr(h, name).argtypes = args
            getattr(h, name).restype = i32
        _hip = h
    return _hip


def check(rc, what):
    assert rc == 0, f"{what}: HIP error {rc}"


def dmalloc(nbytes):
    p = ctypes.c_void_p()
    check(hip().hipMalloc(ctypes.byref(p), max(int(nbytes), 1)), "hipMalloc")
    return p


def upload(ptr, data):
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data).view(np.uint8).reshape(-1)
    if a.size:
        check(hip().hipMemcpy(ptr, a.ctypes.data, a.size, H2D), "hipMemcpy H2D")


def download(ptr, nbytes):
    a = np.empty(int(nbytes), np.uint8)
    if a.size:
        check(hip().hipMemcpy(a.ctypes.data, ptr, a.size, D2H), "hipMemcpy D2H")
    return a


def sync():
    check(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")


class Arena:
    """One hipMalloc holding `specs` (see layout()), every guard filled with a seeded pattern.  Use as a context manager: freed on exit."""

    def __init__(self, specs, seed=0, guard=GUARD):
        self.slots, self.total = layout(specs, guard)
        self.by = {s.name: s for s in self.slots}
        assert len(self.by) == len(self.slots), "buffer names must be unique"
        self.base = dmalloc(self.total)
        assert self.base.value % 256 == 0
        self.pattern = np.random.default_rng(seed).integers(0, 256, guard + 512, dtype=np.uint8)
        for s in self.slots:
            self._put(s.lo, self.pattern[: s.off - s.lo])
            self._put(s.off + s.nbytes, self.pattern[: s.hi - s.off - s.nbytes])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def free(self):
        if self.base is not None:
            hip().hipDeviceSynchronize()
            hip().hipFree(self.base)
            self.base = None

    def _put(self, off, a):
        upload(self.base.value + off, a)

    def ptr(self, name):
        return self.base.value + self.by[name].off

    def size(self, name):
        return self.by[name].nbytes

    def upload(self, name, data):
        a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert a.size <= self.size(name), (name, a.size, self.size(name))
        upload(self.ptr(name), a)

    def download(self, name, nbytes=None):
        return download(self.ptr(name), self.size(name) if nbytes is None else nbytes)

    def poison(self, name, pattern):
        """Fill the buffer: an int is a byte value, an array / bytes is tiled over it."""
        n = self.size(name)
        if isinstance(pattern, int):
            check(hip().hipMemset(self.ptr(name), pattern, n), "hipMemset")
        else:
            p = np.frombuffer(pattern, np.uint8) if isinstance(pattern, (bytes, bytearray)) else np.asarray(pattern, np.uint8).reshape(-1)
            upload(self.ptr(name), np.resize(p, n))

    def check_guards(self, names=None):
        sync()
        for s in self.slots:
            if names is not None and s.name not in names:
                continue
            front = download(self.base.value + s.lo, s.off - s.lo)
            bad = np.flatnonzero(front != self.pattern[: front.size])
            assert bad.size == 0, f"guard in front of {s.name!r} changed: first at {front.size - bad[-1]} bytes before its start"
            back = download(self.base.value + s.off + s.nbytes, s.hi - s.off - s.nbytes)
            bad = np.flatnonzero(back != self.pattern[: back.size])
            what = "read-only tail" if s.source else "guard"
            assert bad.size == 0, f"{what} behind {s.name!r} changed: first at offset {int(bad[0])} from its end (byte {int(bad[0]) + s.nbytes})"


class Stream:
    """A non-default HIP stream (hipStreamCreate); the `_dev` entry points take it as `void*`."""

    def __init__(self):
        self.s = ctypes.c_void_p()
        check(hip().hipStreamCreate(ctypes.byref(self.s)), "hipStreamCreate")

    @property
    def handle(self):
        return self.s.value

    def synchronize(self):
        check(hip().hipStreamSynchronize(self.s), "hipStreamSynchronize")

    def close(self):
        if self.s is not None:
            hip().hipStreamSynchronize(self.s)
            hip().hipStreamDestroy(self.s)
            self.s = None


def results(hb, raw, k=1):
    """hb_result records from their bytes (a download of k * 32 bytes)."""
    a = bytes(np.asarray(raw, np.uint8)[: 32 * k])
    return [hb.hb_result.from_buffer_copy(a, 32 * i) for i in range(k)]


class PinnedResults:
    """k hb_result records in hb_host_alloc memory (pinned): the device writes them, the host reads them after a synchronisation."""

    def __init__(self, hb, k=1):
        self.hb, self.k = hb, k
        self.ptr = hb.lib().hb_host_alloc(32 * k)
        assert self.ptr, "hb_host_alloc failed"
        ctypes.memset(self.ptr, 0xA5, 32 * k)

    def __getitem__(self, i):
        assert 0 <= i < self.k
        return self.hb.hb_result.from_buffer_copy((ctypes.c_char * 32).from_address(self.ptr + 32 * i))

    def address(self, i=0):
        return self.ptr + 32 * i

    def close(self):
        if self.ptr:
            self.hb.lib().hb_host_free(self.ptr)
            self.ptr = None
