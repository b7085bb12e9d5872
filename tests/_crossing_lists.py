"""What the crossing-list tests and the fixture generator (tests/golden/make_golden_crossing_lists.py) share: the fixture, the host program
tests/cpp/crossing_lists_host.cpp (the header's brute force and the header's walk with an array sink) as a callable, the offsets the tests lay the slots
out with, and the comparison of slots with scene.crossing_slots.  Scenes, rays and records are those of tests/_crossings.py."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _crossings as X
import _host

FIXTURE = os.path.join(_host.ROOT, "tests", "golden", "crossing_lists.npz")
GUARD = 32                          # slots behind the capacity that nothing may touch
POISON = np.uint32(0xFFFFFFFF)
STRIDES = (1, 3, 8, 9, 32)          # below the page, at it, one beyond, above the largest count of the fixture (28)


def fixture_lists(fixture, name: str):
    """(offsets int64, t float32, key int32) of a scene of the fixture"""
    return fixture[name + "_offsets"], fixture[name + "_t"].view(np.float32), fixture[name + "_key"]


def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("crossing_lists_host", directory, sanitize)


def host_lists(exe: str, directory, tris: np.ndarray, rays: np.ndarray, capacity: int, offsets=None, stride: int = 0, grid: dict | None = None, page: int = 8) -> dict:
    """The host program over rays (n, 8).  grid None: the header's brute force; else the header's walk over grid arrays with page capacity `page`.  offsets:
    int64 (n + 1,), or None with stride >= 1.  Returns "t" uint32 bits and "key" int32 (capacity,), "guard" uint32 (GUARD, 2), "records" (n,) HIT_DTYPE,
    "totals" int64[6] (rays, cells, tests, flushes, entries written, rays that did not fit) and "excess"."""
    d = str(directory)
    n = int(rays.shape[0])
    params = struct.pack("<iiqi", n, int(stride), int(capacity), GUARD)
    args = [exe, "brute" if grid is None else "walk", os.path.join(d, "cl_params.bin")]
    if grid is not None:
        params += _host.grid_header(grid) + struct.pack("<i", int(page))
        args += _host.grid_files(d, grid, "cl_")
    with open(args[2], "wb") as f:
        f.write(params)
    out = os.path.join(d, "cl_out.bin")
    off = np.zeros(0, np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    subprocess.run(args + [_host.put(d, "cl_tris", np.ascontiguousarray(tris, dtype=np.float32)), _host.put(d, "cl_rays", np.ascontiguousarray(rays, dtype=np.float32)),
                           _host.put(d, "cl_offsets", off), out], check=True, timeout=900)
    raw = np.fromfile(out, dtype=np.uint8)
    ne = 8 * (capacity + GUARD)
    slots = raw[:ne].view(np.uint32).reshape(-1, 2)
    tail = raw[ne + 16 * n:].view(np.int64)
    return {"t": slots[:capacity, 0].copy(), "key": slots[:capacity, 1].view(np.int32).copy(), "guard": slots[capacity:].copy(),
            "records": raw[ne:ne + 16 * n].view(scene.HIT_DTYPE), "totals": tail[:6].copy(), "excess": int(tail[6])}


def layouts(lists, capacity_slack: int = 5):
    """the CSR layouts of the tests as (name, offsets, capacity): exact; every room one short (never below 0); every room two long; and offsets with one slot to spare per ray and a
    negative, a decreasing and a beyond-capacity pair put in -- rays 3, 2 and the last one then write nothing"""
    lo = lists[0]
    m = lo[1:] - lo[:-1]
    n = m.size

    def scan(room):
        o = np.zeros(n + 1, np.int64)
        np.cumsum(room, out=o[1:])
        return o

    out = [("exact", lo.copy(), int(lo[-1])), ("short", scan(np.maximum(m - 1, 0)), int(np.maximum(m - 1, 0).sum())), ("long", scan(m + 2), int((m + 2).sum()))]
    # one more slot than the list needs for every ray, then three pairs spoilt.  The slots of those rays stay as they were: nobody else owns them.
    bad = scan(m + 1)
    cap = int(bad[-1]) + capacity_slack
    bad[3] = -2                     # ray 2 now ends before it starts (decreasing: room 0), ray 3 starts at -2 (negative: room 0)
    bad[n] = cap + 1                # the last ray ends beyond the capacity: room 0
    out.append(("malformed", bad, cap))
    return out


def assert_slots(got: dict, want: dict, what: str):
    """every slot: the entry scene.crossing_slots expects where a ray owns it, the poison where none does; the guard untouched"""
    w = want["written"]
    assert (got["guard"] == POISON).all(), f"{what}: written beyond the capacity"
    bad = w & ((got["t"] != want["t"]) | (got["key"] != want["key"]))
    assert not bad.any(), f"{what}: {bad.sum()} of {w.sum()} owned slots differ, first at {np.flatnonzero(bad)[:5]}: got {got['t'][bad][:3]}, {got['key'][bad][:3]}, want {want['t'][bad][:3]}, {want['key'][bad][:3]}"
    stray = ~w & ((got["t"] != POISON) | (got["key"] != -1))
    assert not stray.any(), f"{what}: {stray.sum()} slots that no ray owns were written, first at {np.flatnonzero(stray)[:5]}"
    if "totals" in got:
        assert int(got["totals"][4]) == want["count"] and int(got["totals"][5]) == want["short"], f"{what}: entries written / rays short {got['totals'][4:6]}, want {want['count']}, {want['short']}"


def rays_that_differ(a: dict, b: dict, offsets) -> np.ndarray:
    """(n,) bool: the record or any slot of the ray differs between two results laid out by the same offsets"""
    bad = (X.rec_bits(a["records"]) != X.rec_bits(b["records"])).any(axis=1)
    slot_bad = (a["t"] != b["t"]) | (a["key"] != b["key"])
    cum = np.concatenate([[0], np.cumsum(slot_bad)])
    o = np.asarray(offsets, np.int64)
    return bad | (cum[o[1:]] - cum[o[:-1]] > 0)
