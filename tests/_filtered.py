"""What the filtered-traversal tests (tests/test_filtered_cpu.py, tests/test_filtered_gpu.py) share: the filters laid over the scenes and rays of the
multi-hit fixture tests/golden/multi_hit.npz, the answer derived from that fixture's eight slots, the brute force scene.filtered_hits computed once per
scene and combination, the any-hit contract, and the host walk tests/cpp/filtered_host.cpp as a callable."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _host
import _multi_hit as M
from _host import bits

KMAX = M.KMAX
SCENES = M.SCENES
RAY_MASKS = (0xFFFFFFFF, 0x1B, 0x06, 0x3F, 0, 0x15, 0x80000000)
# what the fixture's eight slots cannot decide is bounded by its full lists (tests/test_multi_hit_cpu.py pins 83 and 7 of them)
UNDECIDED_CAP = {"soup": 83, "mesh": 7}
MIN_FIRST_SLOT_CHANGED = {"soup": 400, "mesh": 150}
MIN_NON_EMPTY = 1000
COMBOS = {"both": (True, True), "filters": (True, False), "masks": (False, True), "neither": (False, False)}       # (filters given, tri_masks given)


def tri_masks(num_tris: int) -> np.ndarray:
    """uint32 per triangle: 0 when j % 7 == 3, else bit j % 5, and bit 5 when j % 11 == 0"""
    j = np.arange(num_tris, dtype=np.int64)
    m = (np.int64(1) << (j % 5)) | np.where(j % 11 == 0, 0x20, 0)
    return np.where(j % 7 == 3, 0, m).astype(np.uint32)


def make_filters(n: int, num_tris: int, slot0: np.ndarray, slot1: np.ndarray) -> np.ndarray:
    """(n, 2) int32 filter records (the mask's 32 bits, skip).  Masks cycle through RAY_MASKS by i % 7.  skip by i % 4: -1; the ray's unfiltered slot-0 id
    (-1 on a miss); its slot-1 id; (i * 7919) % num_tris.  Of the rays with i % 4 == 0 every sixteenth carries another negative value: they all skip nothing."""
    i = np.arange(n, dtype=np.int64)
    mask = np.asarray(RAY_MASKS, dtype=np.int64)[i % 7]
    skip = np.full(n, -1, dtype=np.int64)
    skip[i % 4 == 1] = np.asarray(slot0, np.int64)[i % 4 == 1]
    skip[i % 4 == 2] = np.asarray(slot1, np.int64)[i % 4 == 2]
    skip[i % 4 == 3] = (i[i % 4 == 3] * 7919) % num_tris
    other = np.asarray([-2, -7, -2147483648, -65536], dtype=np.int64)
    sel = i % 64 == 0
    skip[sel] = other[(i[sel] // 64) % 4]
    f = np.empty((n, 2), dtype=np.int32)
    f[:, 0] = mask.astype(np.uint32).view(np.int32)
    f[:, 1] = skip.astype(np.int32)
    return f


def all_ones_filters(n: int) -> np.ndarray:
    f = np.empty((n, 2), dtype=np.int32)
    f[:, 0] = -1; f[:, 1] = -1
    return f


class Inputs:
    pass


_INPUTS, _WANTED = {}, {}


def inputs(name: str) -> Inputs:
    """one scene of the fixture with the filters over it; made once per process and left unchanged"""
    if name not in _INPUTS:
        fx = np.load(M.FIXTURE)
        c = Inputs()
        c.name = name
        c.tris = M.make_tris(name)
        c.num_tris = c.tris.shape[0]
        c.rays, c.ids, c.t = fx[name + "_rays"], fx[name + "_ids"], fx[name + "_t"]
        c.n = c.rays.shape[0]
        c.filters = make_filters(c.n, c.num_tris, c.ids[:, 0], c.ids[:, 1])
        c.tri_masks = tri_masks(c.num_tris)
        _INPUTS[name] = c
    return _INPUTS[name]


def combo_args(c: Inputs, combo: str):
    """(filters | None, tri_masks | None) of one of COMBOS"""
    f, m = COMBOS[combo]
    return (c.filters if f else None), (c.tri_masks if m else None)


def wanted(name: str, combo: str = "both"):
    """(ids, t) of scene.filtered_hits for k = 8 over all rays of the scene (the list for k is its first k columns); computed once, left unchanged"""
    if (name, combo) not in _WANTED:
        c = inputs(name)
        f, m = combo_args(c, combo)
        ids, t = scene.filtered_hits(c.tris, c.rays, KMAX, f, m)
        ids.setflags(write=False); t.setflags(write=False)
        _WANTED[(name, combo)] = (ids, t)
    return _WANTED[(name, combo)]


def from_fixture(c: Inputs, k: int, filters=None, masks=None):
    """The filter applied to the fixture's eight slots: (ids (n, k), t (n, k), decided (n,)).  A ray is DECIDED for k when its unfiltered list has fewer than
    8 entries (the fixture holds all its intersections) or at least k entries survive."""
    n = c.n
    rows = np.repeat(np.arange(n), KMAX).reshape(n, KMAX)
    used = c.ids >= 0
    keep = used & scene.takes_part(rows, np.where(used, c.ids, 0), filters, masks)
    order = np.argsort(~keep, axis=1, kind="stable")                  # the survivors first, in their order
    ids = np.where(np.take_along_axis(keep, order, axis=1), np.take_along_axis(c.ids, order, axis=1), -1)[:, :k]
    t = np.where(np.take_along_axis(keep, order, axis=1), np.take_along_axis(c.t, order, axis=1), c.rays[:, 7:8])[:, :k].astype(np.float32)
    decided = (used.sum(axis=1) < KMAX) | (keep.sum(axis=1) >= k)
    return ids.astype(np.int32), t, decided


def lists_differ(ids, t, want_ids, want_t) -> np.ndarray:
    """(n,) bool: a ray's ids or t bits differ in some slot"""
    return (np.asarray(ids) != np.asarray(want_ids)).any(axis=1) | (bits(t) != bits(want_t)).any(axis=1)


def assert_lists(got, want_ids, want_t, what: str, only=None):
    """got: (n, k) HIT_DTYPE; ids equal, t bit-equal on every ray (or on the rays of the mask `only`)"""
    k = got.shape[1]
    bad = lists_differ(got["id"], got["t"], want_ids[:, :k], want_t[:, :k])
    if only is not None:
        bad &= only
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} rays differ, first at {np.flatnonzero(bad)[:5]}"


def assert_filter_bites(c: Inputs):
    """a filter that is ignored, or one that rejects everything, cannot pass"""
    ids, _ = wanted(c.name, "both")
    changed = (ids[:, 0] != c.ids[:, 0]).sum()
    assert changed >= MIN_FIRST_SLOT_CHANGED[c.name], f"{c.name}: the filter changes the first slot of {changed} rays only"
    assert (ids[:, 0] >= 0).sum() >= MIN_NON_EMPTY
    assert (c.filters[:, 1] < -1).sum() >= 4, "negative skips other than -1 are among the filters"


def assert_any_hit(got, tris, rays, filters, masks, first_ids, what: str):
    """The any-hit contract.  got: (n,) HIT_DTYPE; first_ids: slot 0 of the k = 1 lists.  id >= 0 exactly where the list is not empty; (id, t) is a candidate of
    the ray: the pair alone is accepted (scene.ray_tri_pairs) with that t bit for bit, and the triangle takes part."""
    got = np.asarray(got).reshape(-1)
    assert ((got["id"] >= 0) == (np.asarray(first_ids) >= 0)).all(), f"{what}: a hit exactly where the candidate set is not empty"
    hit = np.flatnonzero(got["id"] >= 0)
    assert (got["id"][hit] < tris.shape[0]).all()
    p = scene.ray_tri_pairs(tris[got["id"][hit]], rays[hit])
    assert p["accept"].all(), f"{what}: the reported pair is an intersection"
    assert (bits(p["t"]) == bits(got["t"][hit])).all(), f"{what}: t is the pair's own t"
    assert scene.takes_part(hit, got["id"][hit], filters, masks).all(), f"{what}: the reported triangle takes part"
    miss = got["id"] < 0
    assert (got["id"][miss] == -1).all() and (bits(got["t"][miss]) == bits(rays[miss, 7])).all(), f"{what}: a miss holds id -1 and the ray's tmax"


def self_exclusion_rays(c: Inputs):
    """Rays that start ON their triangle: for every primary ray of the fixture with a hit, origin = its hit point (float32), tmin = 0, tmax = inf, direction =
    the primary direction mirrored at the triangle's plane.  Returns (rays (m, 8), the triangle each starts on (m,) int32)."""
    primary = np.flatnonzero(c.ids[:48 * 48, 0] >= 0)
    r = c.rays[primary]
    own = c.ids[primary, 0].astype(np.int32)
    d = r[:, 4:7]
    n = c.tris[own][:, [3, 7, 11]].astype(np.float32)
    dn = ((d * n).sum(axis=1) / (n * n).sum(axis=1)).astype(np.float32)
    out = np.zeros((primary.size, 8), dtype=np.float32)
    out[:, 0:3] = r[:, 0:3] + c.t[primary, 0:1] * d
    out[:, 4:7] = d - np.float32(2.0) * dn[:, None] * n
    out[:, 7] = np.float32(np.inf)
    return out, own


def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("filtered_host", directory, sanitize)


def host_walk(exe: str, directory, grid: dict, tris: np.ndarray, rays: np.ndarray, k: int, filters=None, masks=None, any_hit: bool = False) -> np.ndarray:
    """The filtered host walk over grid arrays (what api.Grid.download returns); filters (n, 2) int32 or None, masks (num_tris,) uint32 or None; the hits as an
    (n, k) HIT_DTYPE array."""
    d = str(directory)
    n = rays.shape[0]
    par = os.path.join(d, "filtered_params.bin")
    with open(par, "wb") as f:
        f.write(_host.grid_header(grid) + struct.pack("<iiiii", k, n, 1 if any_hit else 0, 0 if filters is None else 1, 0 if masks is None else 1))
    out = os.path.join(d, "filtered_out.bin")
    f_file = _host.put(d, "filters", np.zeros((0, 2), np.int32) if filters is None else np.ascontiguousarray(filters, dtype=np.int32))
    m_file = _host.put(d, "tri_masks", np.zeros(0, np.uint32) if masks is None else np.ascontiguousarray(masks, dtype=np.uint32))
    subprocess.run([exe, "walk", par, *_host.grid_files(d, grid), _host.put(d, "tris", np.ascontiguousarray(tris, dtype=np.float32)),
                    _host.put(d, "rays", np.ascontiguousarray(rays, dtype=np.float32)), f_file, m_file, out], check=True, timeout=600)
    return np.fromfile(out, dtype=scene.HIT_DTYPE).reshape(n, k)
