"""What the fill tests (hagrid_fill_lattice: test_fill_lattice_cpu.py, test_fill_lattice_gpu.py) and the fixture generator
(tests/golden/make_golden_fill_lattice.py) share: the scenes and lattices of the fixture, the analytic truth of the box scenes, the fixture's keys, and the host
program tests/cpp/fill_lattice_host.cpp (the header's brute force and the header's walk with the row sink) as a callable."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _crossings as X
import _host

FIXTURE = os.path.join(_host.ROOT, "tests", "golden", "fill_lattice.npz")
SCENES = ("solids", "soup", "mesh", "boxes", "open_box")
MASKS = (1, 2, 3, 4, 5, 6, 7)
PAGES = (1, 2, 4, 8)
BOXES = (((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((1.5, 0.25, 0.25), (2.5, 0.75, 1.0)))
NEAR = 0.03                         # solids: the tessellation lies closer than this to the analytic surface (X.BAND of the smallest radius)


def box_tris(lo, hi) -> np.ndarray:
    """the twelve triangles of an axis-aligned box, each face split along a diagonal, the stored normals pointing outwards"""
    lo = np.asarray(lo, np.float32); hi = np.asarray(hi, np.float32)
    corner = lambda i: np.where([i & 1, i & 2, i & 4], hi, lo).astype(np.float32)
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]        # -x, +x, -y, +y, -z, +z
    centre = (lo + hi) * np.float32(0.5)
    v = []
    for q in quads:
        for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
            a, b, c = (corner(i) for i in tri)
            n = np.cross(a - b, c - a)                      # the stored normal of tris_from_vertices
            if np.dot(n, (a + b + c) / 3 - centre) < 0:
                b, c = c, b
            v.append((a, b, c))
    v = np.asarray(v, np.float32)
    return scene.tris_from_vertices(v[:, 0], v[:, 1], v[:, 2])


def make_tris(name: str) -> np.ndarray:
    if name == "boxes":
        return np.ascontiguousarray(np.concatenate([box_tris(*b) for b in BOXES]))
    if name == "open_box":
        return np.ascontiguousarray(box_tris(*BOXES[0])[:-1])
    return X.make_tris(name)


def _over_box(tris, n, grow):
    lo, hi = scene.tris_bbox(tris)
    ext = (hi - lo).astype(np.float32)
    n = np.array(n, np.int32)
    o = (lo - np.float32(0.5 * grow) * ext).astype(np.float32)
    return o, ((ext * np.float32(1.0 + grow)) / n.astype(np.float32)).astype(np.float32), n


def lattices(name: str, tris: np.ndarray) -> list:
    """the lattices of a scene as (key, origin, size, n)"""
    f3 = lambda v: np.full(3, v, np.float32)
    if name == "solids":
        s = [q for q in scene.make_closed_solids(X.DETAIL)[1] if q["kind"] == "sphere"][0]
        r = np.float32(s["radii"][0])
        brick = ((np.asarray(s["centre"], np.float32) - np.float32(0.2) * r).astype(np.float32), f3(r / np.float32(4.0)), np.array((9, 7, 5), np.int32))
        return [("solids_a", *_over_box(tris, (24, 20, 28), 0.1)), ("solids_brick", *brick)]
    if name in ("soup", "mesh"):
        return [(name + "_a", *_over_box(tris, (12, 10, 14), 0.1))]
    out = [(name + "_a", f3(-0.5), f3(0.25), np.array((14, 8, 8), np.int32)), (name + "_b", f3(-0.625), f3(0.25), np.array((14, 8, 8), np.int32)),
           (name + "_c", f3(-0.5625), f3(0.125), np.array((28, 16, 16), np.int32))]
    if name == "boxes":
        out += [("boxes_one", f3(0.25), f3(0.5), np.array((1, 1, 1), np.int32)),
                ("boxes_flat", np.float32([-0.4, 0.1, -0.3]), np.float32([0.7, 0.8, 0.6]), np.array((5, 1, 3), np.int32))]
    return out


def all_cases():
    """(scene name, key, origin, size, n) of every lattice of the fixture"""
    return [(name, *lat) for name in SCENES for lat in lattices(name, make_tris(name))]


def centres(origin, size, n) -> np.ndarray:
    return np.ascontiguousarray(scene.lattice_centres(origin, size, n)["p"])


def boxes_truth(points: np.ndarray, boxes=BOXES):
    """(inside (n,) int32, on_surface (n,) bool) of points against the closed axis-aligned boxes, exactly (the corners are float32 values)"""
    p = np.asarray(points, np.float64)
    inside = np.zeros(p.shape[0], bool); on = np.zeros(p.shape[0], bool)
    for lo, hi in boxes:
        lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64)
        closed = ((p >= lo) & (p <= hi)).all(axis=1)
        strict = ((p > lo) & (p < hi)).all(axis=1)
        inside |= strict; on |= closed & ~strict
    return inside.astype(np.int32), on


def solids_truth(points: np.ndarray):
    """(inside (n,) int32, distance to the nearest analytic surface (n,) float64) of points against the closed solids"""
    solids = scene.make_closed_solids(X.DETAIL)[1]
    d = np.stack([scene.solid_distance(s, points) for s in solids])
    return ((d < 0).sum(axis=0) & 1).astype(np.int32), np.abs(d).min(axis=0)


def row_counts(n) -> tuple:
    nx, ny, nz = (int(v) for v in n)
    return ny * nz, nx * nz, nx * ny


def rows_of_mask(n, mask: int) -> np.ndarray:
    """the indices, into the records of all three axes, of the rows of the axes in `mask`, in the order hagrid_fill_lattice writes them"""
    rc = row_counts(n)
    first = (0, rc[0], rc[0] + rc[1])
    return np.concatenate([np.arange(first[a], first[a] + rc[a]) for a in range(3) if mask & (1 << a)])


def fixture_case(fx, key: str, mask: int, winding: bool) -> dict:
    """what the fixture holds of one lattice, one axis mask and one vote rule: "inside" int32 per voxel, "records" (rows, 4) uint32 and "abstained" bool of the
    mask's rows"""
    n = fx[key + "_n"]
    rows = rows_of_mask(n, mask)
    return {"inside": fx[key + "_inside"][1 if winding else 0, mask - 1].astype(np.int32), "records": fx[key + "_records"][rows],
            "abstained": fx[key + "_abstained"][1 if winding else 0][rows] != 0}


# ---- tests/cpp/fill_lattice_host.cpp ------------------------------------------------------------------------------------------------

def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("fill_lattice_host", directory, sanitize)


def host_fill(exe: str, directory, tris: np.ndarray, origin, size, n, axes: int = 7, winding: bool = False, grid: dict | None = None, page: int = 8) -> dict:
    """The host program over a lattice.  grid None: the header's fill_row (brute force); else the header's walk over grid arrays with page capacity `page`.
    Returns "inside" int32 per voxel, "records" (rows, 4) uint32, "abstained" bool per row, "totals" int64[5] (rows, cells, tests, flushes, abstained)."""
    d = str(directory)
    params = struct.pack("<3f3f3iii", *[float(v) for v in origin], *[float(v) for v in size], *[int(v) for v in n], int(axes), 1 if winding else 0)
    par = os.path.join(d, "fl_params.bin")
    args = [exe, "brute" if grid is None else "walk", par]
    if grid is not None:
        params += _host.grid_header(grid) + struct.pack("<i", int(page))
        args += _host.grid_files(d, grid, "fl_")
    with open(par, "wb") as f:
        f.write(params)
    out = os.path.join(d, "fl_out.bin")
    subprocess.run(args + [_host.put(d, "fl_tris", np.ascontiguousarray(tris, dtype=np.float32)), out], check=True, timeout=900)
    raw = np.fromfile(out, dtype=np.uint8)
    voxels = int(np.prod([int(v) for v in n]))
    rows = rows_of_mask(n, int(axes) or 7).size
    a, b = 4 * voxels, 4 * voxels + 16 * rows
    pad = (rows + 7) // 8 * 8
    return {"inside": raw[:a].view(np.int32).copy(), "records": raw[a:b].view(np.uint32).reshape(rows, 4).copy(), "abstained": raw[b:b + rows] != 0,
            "totals": raw[b + pad:].view(np.int64)[:5].copy()}


def assert_fill_equal(got: dict, want: dict, what: str):
    """inside, records and abstained rows, bit for bit"""
    bad = got["inside"] != want["inside"]
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} voxels differ, first at {np.flatnonzero(bad)[:5]}: got {got['inside'][bad][:5]}, want {want['inside'][bad][:5]}"
    if got.get("records") is not None:
        X.assert_records_equal(got["records"], want["records"], what)
    if got.get("abstained") is not None:
        assert (got["abstained"] == want["abstained"]).all(), f"{what}: the abstaining rows differ"
