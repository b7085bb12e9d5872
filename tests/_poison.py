"""Poisoned, guarded output buffers for the GPU tests (testing: "compared outputs are poisoned and guarded").

A launch whose output is compared afterwards writes into memory that was filled with ones (every byte 0xFF) after the previous write to it, so a
record the launch skipped cannot pass for a record it wrote: the pool of a `keep` manager hands back the slot the previous launch's (correct) answers
still lie in, and a loop over one buffer sees the previous iteration's.  An untouched Hit reads id = -1 and t, u, v = 0xFFFFFFFF (a NaN): a real miss
has t = tmax, a real hit id >= 0, so the bit-for-bit comparison of t with the oracle fails on it, and so do u == 0 and v == 0.  Behind the payload lie
`guard` more bytes of ones that no launch may touch.

    d = alloc_out(mem, nbytes)            # nbytes + guard, all ones
    ... launch ...
    got = fetch(mem, d, dtype, count)     # payload; asserts the guard
    poison(mem, d, nbytes)                # before the next compared launch into the same buffer
    mem.free(d)

Tests that compare only part of a record (ids without t, counts) call assert_all_written on what they fetched."""
import numpy as np

GUARD = 256


def alloc_out(mem, nbytes, guard=GUARD):
    """a buffer of nbytes + guard bytes, every byte 0xFF"""
    nbytes = int(nbytes)
    p = mem.alloc(nbytes + guard)
    mem.one(p, nbytes + guard)
    return p


def poison(mem, ptr, nbytes, guard=GUARD):
    """refills payload and guard with ones: before a repeated launch into the same buffer"""
    mem.one(ptr, int(nbytes) + guard)


def check_guard(guard_bytes):
    g = np.ascontiguousarray(guard_bytes).view(np.uint8).reshape(-1)
    bad = np.flatnonzero(g != 0xFF)
    assert bad.size == 0, f"written beyond the buffer: {bad.size} guard bytes changed, the first {bad[0]} bytes behind the payload"


def fetch(mem, ptr, dtype, count, guard=GUARD):
    """downloads `count` records of `dtype` and the guard behind them; the guard must still be all ones; returns the payload"""
    dtype = np.dtype(dtype)
    nbytes = dtype.itemsize * int(count)
    raw = mem.download(ptr, np.uint8, nbytes + guard)
    check_guard(raw[nbytes:])
    return raw[:nbytes].view(dtype)


def assert_all_written(records):
    """no record (an element of a structured or 1-D word array, a row of a 2-D one) is still entirely 0xFF"""
    a = np.ascontiguousarray(records)
    if a.size == 0:
        return
    raw = a.view(np.uint8).reshape(a.shape[0], -1)
    for word in (np.uint64, np.uint32, np.uint16):                   # (the widest word a record is made of: the 16M-ray batches are looked at in two words per hit)
        if raw.shape[1] % np.dtype(word).itemsize == 0 and raw.ctypes.data % np.dtype(word).itemsize == 0:
            raw = raw.view(word); break
    untouched = np.flatnonzero((raw == np.iinfo(raw.dtype).max).all(axis=1))
    assert untouched.size == 0, f"{untouched.size} of {a.shape[0]} records never written, first at {untouched[:5]}"
