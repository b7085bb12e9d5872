"""What the box-overlap tests and the fixture generator (tests/golden/make_golden_overlap.py) share: the scenes and boxes of the fixture
tests/golden/overlap.npz (regenerated, not stored: counter-based generators of hagrid_amd/scene.py) and the host program tests/cpp/overlap_host.cpp as
callables (the triangle / box test per pair, the brute-force definition, the walk over grid arrays)."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _host
from _host import ROOT, INC, oracle_grid, oracle_grid_arrays                # names the tests use

FIXTURE = os.path.join(ROOT, "tests", "golden", "overlap.npz")
SCENES = ("soup", "mesh")
NUM_BOXES = 4096
KMAX = 8
KS = (1, 2, 3, 5, 8)
# the sections of the 4096 boxes of a scene
ONE, FINE, FIVE, TWENTY, LATTICE, POINT, PAGED, SPECIAL = (slice(0, 1536), slice(1536, 2048), slice(2048, 2816), slice(2816, 3072), slice(3072, 3584),
                                                           slice(3584, 3840), slice(3840, 3968), slice(3968, 4096))
PAGED_FROM = 2048                        # box PAGED.start + i repeats box PAGED_FROM + i with first = (third id of that box's answer) + 1
BOX_SEED = 0x6F7665726C6170              # "overlap"
NUM_UNBOUNDED = 384                      # boxes with infinite bounds per scene, beside the 4096 (unbounded_boxes)
NUM_PAIRS = 2048                         # (triangle, box) pairs per scene pinned to the reference

_u = scene._uniform_rows


def make_tris(name: str) -> np.ndarray:
    return scene.make_soup(20000, seed=7) if name == "soup" else scene.make_stadium(0.05)


def boxes_around(centres: np.ndarray, edge) -> np.ndarray:
    """(n, 8) float32 box rows: centre -+ edge / 2 per axis (edge: a scalar, (n,) or (n, 3)), first = 0"""
    c = np.asarray(centres, np.float32)
    h = (np.broadcast_to(np.asarray(edge, np.float32).reshape(-1, 1) if np.ndim(edge) == 1 else np.asarray(edge, np.float32), c.shape) * np.float32(0.5)).astype(np.float32)
    b = np.zeros((c.shape[0], 8), dtype=np.float32)
    b[:, 0:3] = c - h; b[:, 4:7] = c + h
    return b


def mixed_centres(tris, lo, hi, count: int, seed: int) -> np.ndarray:
    """two thirds near the surface (1 % of the diagonal), one third uniform in the box enlarged by 10 %"""
    near = (2 * count) // 3
    return np.concatenate([scene.make_points_near_surface(tris, lo, hi, near, seed), scene.make_points_uniform(lo, hi, count - near, seed + 1)])


def vertices_of(tris: np.ndarray, count: int, seed: int) -> np.ndarray:
    u = _u(seed, count, 2)
    j = np.minimum((u[:, 0] * np.float32(tris.shape[0])).astype(np.int64), tris.shape[0] - 1)
    which = np.minimum((u[:, 1] * np.float32(3.0)).astype(np.int64), 2)
    t = tris[j]
    return np.where((which == 0)[:, None], t[:, 0:3], np.where((which == 1)[:, None], t[:, 0:3] - t[:, 4:7], t[:, 0:3] + t[:, 8:11])).astype(np.float32)


def special_boxes(tris, lo, hi) -> np.ndarray:
    """128 boxes: [0] the whole scene box; [1:7] straddling each face of the grid; [7:13] beyond each face; [13:21] far outside; [21:29] min > max on an
    axis; [29:37] a NaN bound; [37] infinite in every direction; [38:41] infinite along one axis; [41:47] half-infinite (one bound infinite); [47:53] a
    half space; [53:56] both bounds of an axis +inf; [56:128] edges from 0.1 % to 50 % of the diagonal around points of the box enlarged by a half"""
    diag = scene.bbox_diagonal(lo, hi)
    inf = np.float32(np.inf)
    centre = ((lo + hi) * np.float32(0.5)).astype(np.float32)
    s = np.zeros((128, 8), dtype=np.float32)
    s[0, 0:3] = lo; s[0, 4:7] = hi
    on = scene.make_points_uniform(lo, hi, 12, BOX_SEED + 20, enlarge=0.0)
    for i in range(12):
        a, up = i % 3, (i // 3) % 2 == 0
        off = np.float32(0.0) if i < 6 else np.float32(0.05) * diag
        on[i, a] = hi[a] + off if up else lo[a] - off
    s[1:13] = boxes_around(on, np.float32(0.04) * diag)
    d = np.float32(2.0) * _u(BOX_SEED + 21, 8, 3) - np.float32(1.0)
    s[13:21] = boxes_around(centre + d * (np.float32(100.0) * diag), np.float32(0.01) * diag)
    base = boxes_around(mixed_centres(tris, lo, hi, 40, BOX_SEED + 22), np.float32(0.05) * diag)
    s[21:29] = base[0:8]
    for i in range(8):
        a = i % 3
        s[21 + i, a], s[21 + i, 4 + a] = s[21 + i, 4 + a], s[21 + i, a]
    s[29:37] = base[8:16]
    for i in range(8):
        s[29 + i, (0, 1, 2, 4, 5, 6)[i % 6]] = np.float32(np.nan)
    s[37, 0:3] = -inf; s[37, 4:7] = inf
    s[38:41] = base[16:19]
    for a in range(3):
        s[38 + a, a] = -inf; s[38 + a, 4 + a] = inf
    s[41:47] = base[19:25]
    for i in range(6):
        a = i % 3
        if i < 3: s[41 + i, a] = -inf
        else:     s[41 + i, 4 + a] = inf
    for i in range(6):
        a = i % 3
        s[47 + i, 0:3] = -inf; s[47 + i, 4:7] = inf
        if i < 3: s[47 + i, 4 + a] = centre[a]
        else:     s[47 + i, a] = centre[a]
    s[53:56] = base[25:28]
    for a in range(3):
        s[53 + a, a] = inf; s[53 + a, 4 + a] = inf
    u = _u(BOX_SEED + 23, 72, 6)
    edge = (np.float32(0.001) * diag) * np.ldexp(np.float32(1.0) + u[:, 0:3], (u[:, 3:6] * np.float32(8.0)).astype(np.int32)).astype(np.float32)   # 0.1 % .. 51 %, no libm
    s[56:128] = boxes_around(scene.make_points_uniform(lo, hi, 72, BOX_SEED + 24, enlarge=0.5), edge)
    return s


def unbounded_boxes(tris: np.ndarray, count: int, seed: int) -> np.ndarray:
    """(count, 8) box rows of 1 % to 7 % of the diagonal (centres as in the fixture) with bounds taken away: of every six boxes, four have one bound
    infinite (each of the six faces in turn), one has two bounds on different axes infinite, one is infinite both ways along one axis.  The finite end
    faces of such boxes lie inside the scene: the case in which a test handed the infinite bounds as they are accepts triangles that have no point in
    the box."""
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    u = _u(seed, count, 3)
    b = boxes_around(mixed_centres(tris, lo, hi, count, seed + 1), (np.float32(0.01) + np.float32(0.06) * u[:, 0]) * diag)
    inf = np.float32(np.inf)
    col = (0, 1, 2, 4, 5, 6)
    for i in range(count):
        f = int(u[i, 1] * np.float32(6.0)) % 6
        kind = i % 6
        b[i, col[f]] = -inf if f < 3 else inf
        if kind == 4:                                   # a second bound, on another axis
            g = (f % 3 + 1 + int(u[i, 2] * np.float32(2.0)) % 2) % 3 + (3 if u[i, 2] >= np.float32(0.5) else 0)
            b[i, col[g]] = -inf if g < 3 else inf
        elif kind == 5:                                 # both bounds of the axis
            b[i, col[f % 3]] = -inf; b[i, col[f % 3 + 3]] = inf
    return b


def fixture_boxes(tris: np.ndarray, paged_ids=None) -> np.ndarray:
    """The 4096 boxes of a scene as (4096, 8) float32 rows (`first` in column 3 as int32 bits): 1536 of 1 % of the diagonal, 512 of 0.2 %, 768 of 5 %, 256 of
    20 % (centres: two thirds near the surface, one third uniform), the 512 voxels of an 8 x 8 x 8 lattice over the scene box, 256 of no extent (128 surface
    samples, 128 vertices), 128 that repeat boxes 2048 .. 2175 with first = (paged_ids[i, 2], the third id of that box's answer) + 1, 128 special
    (special_boxes).  paged_ids None: those 128 keep first = 0 (the generator's first pass)."""
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    b = np.zeros((NUM_BOXES, 8), dtype=np.float32)
    for k, (sec, frac) in enumerate(((ONE, 0.01), (FINE, 0.002), (FIVE, 0.05), (TWENTY, 0.2))):
        b[sec] = boxes_around(mixed_centres(tris, lo, hi, sec.stop - sec.start, BOX_SEED + 2 * k), np.float32(frac) * diag)
    b[LATTICE] = scene.lattice_boxes(lo, ((hi - lo) / np.float32(8.0)).astype(np.float32), (8, 8, 8)).view(np.float32).reshape(-1, 8)
    pts = np.concatenate([scene.make_points_surface(tris, 128, BOX_SEED + 10)[0], vertices_of(tris, 128, BOX_SEED + 11)])
    b[POINT, 0:3] = pts; b[POINT, 4:7] = pts
    b[PAGED] = b[PAGED_FROM:PAGED_FROM + 128]
    if paged_ids is not None:
        b[PAGED, 3] = (np.asarray(paged_ids)[:, 2].astype(np.int32) + 1).view(np.float32)
    b[SPECIAL] = special_boxes(tris, lo, hi)
    return b


def box_sum(boxes: np.ndarray) -> int:
    return int(np.ascontiguousarray(boxes).view(np.uint32).astype(np.uint64).sum())


def scene_boxes(fixture, name: str, tris: np.ndarray) -> np.ndarray:
    """the boxes of a scene, the paged ones from the fixture's answers; checked against the fixture's checksum"""
    b = fixture_boxes(tris, fixture[name + "_ids"][PAGED_FROM:PAGED_FROM + 128])
    assert box_sum(b) == int(fixture[name + "_box_sum"]), "the fixture's boxes are the generators' boxes"
    return b


def expected(fixture, name: str, k: int):
    """(ids (n, k), counts) of a scene for k, from |S| and the first 8 ids"""
    ids = np.ascontiguousarray(fixture[name + "_ids"][:, :k]).astype(np.int32)
    return ids, np.minimum(fixture[name + "_sizes"], k + 1).astype(np.int32)


def bounds_check(tris: np.ndarray, boxes: np.ndarray) -> np.ndarray:
    """triangle i against box i: do the bounding intervals overlap on every axis (the three box axes of the separating-axis test)?"""
    T = np.asarray(tris, np.float32); B = np.ascontiguousarray(boxes).view(np.float32).reshape(-1, 8)
    v0 = T[:, 0:3]; v1 = v0 - T[:, 4:7]; v2 = v0 + T[:, 8:11]
    tmin = np.fmin(v0, np.fmin(v1, v2)); tmax = np.fmax(v0, np.fmax(v1, v2))
    return ~((tmin > B[:, 4:7]) | (tmax < B[:, 0:3])).any(axis=1)


# ---- tests/cpp/overlap_host.cpp -------------------------------------------------------------------------------------------------

def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("overlap_host", directory, sanitize)


_put = _host.put


def _rows(boxes) -> np.ndarray:
    return np.ascontiguousarray(boxes).view(np.float32).reshape(-1, 8)


def host_pairs(exe: str, directory, tris: np.ndarray, boxes: np.ndarray) -> np.ndarray:
    """triangle i against box i through meets() of include/hagrid/overlap.h"""
    n = tris.shape[0]
    par = os.path.join(str(directory), "pairs_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<i", n))
    out = os.path.join(str(directory), "pairs_out.bin")
    subprocess.run([exe, "pairs", par, _put(directory, "pairs_tris", tris.astype(np.float32)), _put(directory, "pairs_boxes", _rows(boxes)), out], check=True, timeout=600)
    return np.fromfile(out, dtype=np.int32) != 0


def host_brute(exe: str, directory, tris: np.ndarray, boxes: np.ndarray, k: int, any_: bool = False, grid=None):
    """brute_force of include/hagrid/overlap.h, the boxes clipped to the grid box `grid` = (min, max) (None: scene.grid_box(tris)): (ids (n, k), counts)"""
    b = _rows(boxes); n = b.shape[0]
    glo, ghi = scene.grid_box(tris) if grid is None else grid
    par = os.path.join(str(directory), "brute_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<3i3f3f", n, k, 1 if any_ else 0, *[float(v) for v in glo], *[float(v) for v in ghi]))
    ids, counts = os.path.join(str(directory), "brute_ids.bin"), os.path.join(str(directory), "brute_counts.bin")
    subprocess.run([exe, "brute", par, _put(directory, "brute_tris", tris.astype(np.float32)), _put(directory, "brute_boxes", b), ids, counts], check=True, timeout=1200)
    return np.fromfile(ids, dtype=np.int32).reshape(n, k), np.fromfile(counts, dtype=np.int32)


def host_walk(exe: str, directory, grid: dict, tris: np.ndarray, boxes: np.ndarray, k: int, any_: bool = False):
    """overlap_query of include/hagrid/overlap.h over grid arrays (keys entries, ref_ids, cells | small_cells, bbox_min, bbox_max, dims, shift: what
    api.Grid.download returns): (ids (n, k), counts, per-box totals (n, 3) int32: cells visited, tests evaluated, sub-blocks pruned)"""
    d = str(directory)
    b = _rows(boxes); n = b.shape[0]
    par = os.path.join(d, "walk_params.bin")
    with open(par, "wb") as f:
        f.write(_host.grid_header(grid) + struct.pack("<3i", n, k, 1 if any_ else 0))
    ids, counts, totals = os.path.join(d, "walk_ids.bin"), os.path.join(d, "walk_counts.bin"), os.path.join(d, "walk_totals.bin")
    subprocess.run([exe, "walk", par, *_host.grid_files(d, grid), _put(d, "tris", np.ascontiguousarray(tris, dtype=np.float32)), _put(d, "boxes", b), ids, counts, totals],
                   check=True, timeout=1200)
    return np.fromfile(ids, dtype=np.int32).reshape(n, k), np.fromfile(counts, dtype=np.int32), np.fromfile(totals, dtype=np.int32).reshape(n, 3)


def assert_answers_equal(got_ids, got_counts, want_ids, want_counts, what: str):
    assert got_ids.shape == want_ids.shape, f"{what}: {got_ids.shape} against {want_ids.shape}"
    bad = (got_ids != want_ids).any(axis=1)
    assert not bad.any(), f"{what}: the ids of {bad.sum()} of {bad.size} boxes differ, first at {np.flatnonzero(bad)[:5]}: got {got_ids[bad][:2]}, want {want_ids[bad][:2]}"
    if got_counts is not None:
        bad = got_counts != want_counts
        assert not bad.any(), f"{what}: the counts of {bad.sum()} boxes differ, first at {np.flatnonzero(bad)[:5]}: got {got_counts[bad][:5]}, want {want_counts[bad][:5]}"
