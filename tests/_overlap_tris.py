"""What the contact-query tests and the fixture generator (tests/golden/make_golden_overlap_tris.py) share: the exact triangle / triangle test in rational
arithmetic that is the yardstick, the pairs, scenes and queries of the fixture tests/golden/overlap_tris.npz (regenerated, not stored: counter-based
generators of hagrid_amd/scene.py) and the host program tests/cpp/overlap_tris_host.cpp as callables."""
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np

from hagrid_amd import scene

import _host
import _overlap as V
from _host import ROOT, INC, oracle_grid, oracle_grid_arrays                # names the tests use

FIXTURE = os.path.join(ROOT, "tests", "golden", "overlap_tris.npz")
SCENES = V.SCENES
KMAX = 8
KS = (1, 2, 3, 4, 5, 8)
SEED = 0x636F6E74616374                  # "contact"
NUM_LATTICE_PAIRS = 16384                # a quarter coplanar (z = 0 for both), an eighth in parallel planes
NUM_SCENE_PAIRS = 4096
NUM_QUERIES = 4096
# the sections of the 4096 queries of a scene
OWN, MOVED_FINE, MOVED, HUGE, BEYOND, INACTIVE, FLAT, PAGED = (slice(0, 1280), slice(1280, 2304), slice(2304, 3328), slice(3328, 3456), slice(3456, 3584),
                                                               slice(3584, 3680), slice(3680, 3968), slice(3968, 4096))
PAGED_FROM = HUGE.start                  # query PAGED.start + i repeats query PAGED_FROM + i with first = (third id of that query's answer) + 1
LATTICE_TRIS, LATTICE_QUERIES = 4000, 1024

_u = scene._uniform_rows
make_tris = V.make_tris


# ---- the yardstick: exact arithmetic, an edge-against-triangle test with the coplanar case handled in 2-D ----------------------------------------

def _sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def _dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def _orient2(p, q, r): return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])


def _segments_meet2(p, q, r, s):
    d1, d2, d3, d4 = _orient2(r, s, p), _orient2(r, s, q), _orient2(p, q, r), _orient2(p, q, s)
    if ((d1 > 0 and d2 < 0) or (d1 < 0 and d2 > 0)) and ((d3 > 0 and d4 < 0) or (d3 < 0 and d4 > 0)):
        return True

    def on(a, b, c):
        return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])
    return (d1 == 0 and on(r, s, p)) or (d2 == 0 and on(r, s, q)) or (d3 == 0 and on(p, q, r)) or (d4 == 0 and on(p, q, s))


def _in_tri2(T, p):
    o = [_orient2(T[0], T[1], p), _orient2(T[1], T[2], p), _orient2(T[2], T[0], p)]
    return all(x >= 0 for x in o) or all(x <= 0 for x in o)


def _segment_meets_tri(P, Q, T):
    """the closed segment PQ against the closed triangle T (not degenerate), exact for int and Fraction coordinates"""
    n = _cross(_sub(T[1], T[0]), _sub(T[2], T[0]))
    dP, dQ = _dot(n, _sub(P, T[0])), _dot(n, _sub(Q, T[0]))
    if (dP > 0 and dQ > 0) or (dP < 0 and dQ < 0):
        return False
    if dP == 0 and dQ == 0:                                 # in the plane: drop the coordinate the normal is largest in
        k = max(range(3), key=lambda i: abs(n[i]))
        ax = [i for i in range(3) if i != k]
        T2 = [(v[ax[0]], v[ax[1]]) for v in T]; p, q = (P[ax[0]], P[ax[1]]), (Q[ax[0]], Q[ax[1]])
        return _in_tri2(T2, p) or _in_tri2(T2, q) or any(_segments_meet2(p, q, T2[i], T2[(i + 1) % 3]) for i in range(3))
    t = Fraction(dP, dP - dQ)
    X = tuple(P[i] + t * (Q[i] - P[i]) for i in range(3))
    return all(_dot(n, _cross(_sub(T[(i + 1) % 3], T[i]), _sub(X, T[i]))) >= 0 for i in range(3))


def exact_meet(A, B) -> bool:
    """do the closed triangles A and B (three vertices each, int or Fraction coordinates, neither degenerate) share a point?  Two triangles meet exactly
    when an edge of one meets the other."""
    return any(_segment_meets_tri(A[i], A[(i + 1) % 3], B) for i in range(3)) or any(_segment_meets_tri(B[i], B[(i + 1) % 3], A) for i in range(3))


def exact_pairs(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """exact_meet of triangle a[i] and triangle b[i] ((n, 12) float32 Tri rows): the float32 vertices (scene.tri_vertices) read as rationals"""
    va, vb = scene.tri_vertices(a), scene.tri_vertices(b)

    def rat(v):
        return [tuple(Fraction(float(c)) for c in p) for p in v]
    return np.array([exact_meet(rat(x), rat(y)) for x, y in zip(va, vb)], dtype=bool)


# ---- (a) lattice pairs ---------------------------------------------------------------------------------------------------------------------------

def _lattice_coords(seed: int, count: int, width: int, lo: int, hi: int) -> np.ndarray:
    """(count, width) integers in [lo, hi]"""
    return np.minimum((_u(seed, count, width) * np.float32(hi - lo + 1)).astype(np.int64), hi - lo) + lo


def _tris_of(P: np.ndarray) -> np.ndarray:
    P = P.astype(np.float32)
    return scene.tris_from_vertices(P[:, 0], P[:, 1], P[:, 2])


def lattice_pairs():
    """(a, b): 16 384 pairs of Tri rows with integer coordinates |c| <= 16 and non-zero normals; the first quarter coplanar (z = 0 for both), the next
    eighth in parallel planes (z = 0 and z = 0 or 1 or -2), the rest anywhere; half of each class with |c| <= 4, where contacts are frequent"""
    out = []
    for kind, count in ((1, NUM_LATTICE_PAIRS // 4), (2, NUM_LATTICE_PAIRS // 8), (0, NUM_LATTICE_PAIRS - NUM_LATTICE_PAIRS // 4 - NUM_LATTICE_PAIRS // 8)):
        for half, R in enumerate((4, 16)):
            want = count // 2
            P = _lattice_coords(SEED + 10 * kind + half, 2 * want, 18, -R, R).reshape(-1, 2, 3, 3)
            if kind == 1:
                P[:, :, :, 2] = 0
            if kind == 2:
                P[:, 0, :, 2] = 0
                P[:, 1, :, 2] = np.array([0, 1, -2])[np.arange(P.shape[0]) % 3][:, None]
            e1, e2 = P[:, :, 1] - P[:, :, 0], P[:, :, 2] - P[:, :, 0]
            ok = (np.cross(e1, e2) != 0).any(axis=2).all(axis=1)
            P = P[ok][:want]
            assert P.shape[0] == want, "not enough pairs with non-zero normals"
            out.append(P)
    P = np.concatenate(out)
    return _tris_of(P[:, 0]), _tris_of(P[:, 1]), P


def lattice_truth(P: np.ndarray) -> np.ndarray:
    return np.array([exact_meet([tuple(int(c) for c in v) for v in p[0]], [tuple(int(c) for c in v) for v in p[1]]) for p in P], dtype=bool)


# ---- (b) scene pairs -----------------------------------------------------------------------------------------------------------------------------

def grid_eps(tris: np.ndarray) -> np.float32:
    glo, ghi = scene.grid_box(tris)
    return np.float32(max(np.abs(glo).max(), np.abs(ghi).max())) * np.float32(1.52587890625e-05)


def scene_pairs(tris: np.ndarray, seed: int) -> np.ndarray:
    """(4096, 2) int32: pairs (i, j), i != j, among triangles whose bounding boxes come within 2 eps of each other -- up to four partners of triangles
    drawn by the generator"""
    Vx = scene.tri_vertices(tris); lo = Vx.min(axis=1); hi = Vx.max(axis=1)
    n = tris.shape[0]
    eps2 = np.float32(2.0) * grid_eps(tris)
    pick = np.minimum((_u(seed, 4 * NUM_SCENE_PAIRS, 1)[:, 0] * np.float32(n)).astype(np.int64), n - 1)
    pairs = []
    for a in pick:
        m = ((lo <= hi[a] + eps2) & (hi >= lo[a] - eps2)).all(axis=1)
        m[a] = False
        for j in np.flatnonzero(m)[:4]:
            pairs.append((a, j))
        if len(pairs) >= NUM_SCENE_PAIRS:
            break
    assert len(pairs) >= NUM_SCENE_PAIRS
    return np.array(pairs[:NUM_SCENE_PAIRS], dtype=np.int32)


def pair_decision(tris: np.ndarray, pairs: np.ndarray) -> np.ndarray:
    """the full pair decision of the query for (i, j): triangle j meets the grown, clipped box of triangle i AND tri_tri_pairs(i, j)"""
    glo, ghi = scene.grid_box(tris)
    boxes = scene.clip_boxes(scene.query_boxes(tris[pairs[:, 0]], glo, ghi), glo, ghi)
    return scene.overlap_pairs(tris[pairs[:, 1]], boxes) & scene.tri_tri_pairs(tris[pairs[:, 0]], tris[pairs[:, 1]])


# ---- (c) queries ---------------------------------------------------------------------------------------------------------------------------------

def scene_labels(name: str, num_tris: int) -> np.ndarray:
    """(num_tris, 3) int32: the mesh's index triples (make_stadium_mesh's faces); the soup has no mesh: triangle j carries (j, -1, -1), its own name"""
    if name == "mesh":
        faces = scene.make_stadium_mesh(0.05)[1]
        assert faces.shape[0] == num_tris
        return np.ascontiguousarray(faces, np.int32)
    lab = np.full((num_tris, 3), -1, dtype=np.int32)
    lab[:, 0] = np.arange(num_tris)
    return lab


def _moved(tris: np.ndarray, offset) -> np.ndarray:
    """the triangles translated: v0 + offset in float32, edges and normal kept"""
    t = tris.copy()
    t[:, 0:3] = (t[:, 0:3] + np.asarray(offset, np.float32)).astype(np.float32)
    return t


def fixture_queries(name: str, tris: np.ndarray, paged_ids=None):
    """(queries (4096, 12) float32, first (4096,) int32, query_labels (4096, 3) int32) of a scene.  OWN: the scene's own triangles (labels: their own);
    MOVED_FINE / MOVED: triangles of the scene moved by 0.5 % / 5 % of the diagonal; HUGE: lattice-like triangles spanning the grid; BEYOND: triangles
    beyond the grid; INACTIVE: a NaN, an inf, a zero normal; FLAT: axis-aligned ones (a coordinate constant); PAGED: the HUGE ones again with
    first = (paged_ids[i, 2], the third id of that query's answer) + 1.  Labels outside OWN are -1."""
    n = tris.shape[0]
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    ext = (hi - lo).astype(np.float32)
    q = np.zeros((NUM_QUERIES, 12), dtype=np.float32)
    lab = np.full((NUM_QUERIES, 3), -1, dtype=np.int32)
    labels = scene_labels(name, n)

    def pick(sec, seed):
        c = sec.stop - sec.start
        return np.minimum((_u(seed, c, 1)[:, 0] * np.float32(n)).astype(np.int64), n - 1)
    own = pick(OWN, SEED + 100)
    q[OWN] = tris[own]; lab[OWN] = labels[own]
    for sec, frac, seed in ((MOVED_FINE, 0.005, SEED + 101), (MOVED, 0.05, SEED + 102)):
        d = (np.float32(2.0) * _u(seed + 50, sec.stop - sec.start, 3) - np.float32(1.0)) * (np.float32(frac) * diag)
        q[sec] = _moved(tris[pick(sec, seed)], d)
    # huge: three corners on a 5 x 5 x 5 lattice over the scene box enlarged by a half
    c = sec_count = HUGE.stop - HUGE.start
    P = _lattice_coords(SEED + 103, 2 * c, 9, 0, 4).reshape(-1, 3, 3)
    P = P[(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) != 0).any(axis=1)][:c]
    assert P.shape[0] == sec_count
    corners = ((lo - np.float32(0.25) * ext) + P.astype(np.float32) * (np.float32(0.375) * ext)).astype(np.float32)
    q[HUGE] = scene.tris_from_vertices(corners[:, 0], corners[:, 1], corners[:, 2])
    # beyond: scene triangles moved out by 2 to 100 diagonals along an axis direction; the last 16 touch the grid's face region from outside
    c = BEYOND.stop - BEYOND.start
    u = _u(SEED + 104, c, 2)
    d = np.zeros((c, 3), dtype=np.float32)
    axis = np.arange(c) % 3; sign = np.where((np.arange(c) // 3) % 2 == 0, np.float32(1.0), np.float32(-1.0))
    d[np.arange(c), axis] = sign * (np.float32(2.0) + np.float32(98.0) * u[:, 0]) * diag
    q[BEYOND] = _moved(tris[pick(BEYOND, SEED + 105)], d)
    # inactive
    c = INACTIVE.stop - INACTIVE.start
    q[INACTIVE] = tris[pick(INACTIVE, SEED + 106)]
    for i in range(c):
        r = INACTIVE.start + i
        if i % 3 == 0:   q[r, (0, 1, 2, 4, 5, 6, 8, 9, 10, 3)[(i // 3) % 10]] = np.float32(np.nan)
        elif i % 3 == 1: q[r, (0, 5, 10, 7, 2, 4)[(i // 3) % 6]] = np.float32(np.inf) if (i // 3) % 2 else np.float32(-np.inf)
        else:            q[r, 3] = q[r, 7] = q[r, 11] = np.float32(0.0)
    q[INACTIVE.start + 3, 0:3] = np.float32(3.0e38); q[INACTIVE.start + 3, 4:7] = np.float32(-3.0e38)      # finite floats, v0 - e1 is not
    # flat: right triangles in an axis plane through a point near the surface, legs of 0.5 % to 8 % of the diagonal
    c = FLAT.stop - FLAT.start
    pts = scene.make_points_near_surface(tris, lo, hi, c, SEED + 107)
    u = _u(SEED + 108, c, 2)
    legs = (np.float32(0.005) * diag) * (np.float32(1.0) + np.float32(15.0) * u)
    v1 = pts.copy(); v2 = pts.copy()
    axis = np.arange(c) % 3
    v1[np.arange(c), (axis + 1) % 3] += legs[:, 0]; v2[np.arange(c), (axis + 2) % 3] += legs[:, 1]
    q[FLAT] = scene.tris_from_vertices(pts, v1.astype(np.float32), v2.astype(np.float32))
    q[PAGED] = q[PAGED_FROM:PAGED_FROM + (PAGED.stop - PAGED.start)]
    first = np.zeros(NUM_QUERIES, dtype=np.int32)
    if paged_ids is not None:
        first[PAGED] = np.asarray(paged_ids)[:, 2].astype(np.int32) + 1
    return np.ascontiguousarray(q), first, lab


def array_sum(a: np.ndarray) -> int:
    return int(np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum())


def scene_queries(fixture, name: str, tris: np.ndarray):
    """the queries of a scene, the paged ones from the fixture's answers; checked against the fixture's checksum"""
    q, first, lab = fixture_queries(name, tris, fixture[name + "_ids"][PAGED_FROM:PAGED_FROM + (PAGED.stop - PAGED.start)])
    assert array_sum(q) + array_sum(first) + array_sum(lab) == int(fixture[name + "_query_sum"]), "the fixture's queries are the generators' queries"
    return q, first, lab


def expected(fixture, key: str, k: int, first: bool = True):
    """(ids (n, k), counts) of the answers `key` for k, from |S| and the first 8 ids; first False: the queries asked without `first` -- the PAGED section
    then answers as the section it repeats"""
    ids8, sizes = fixture[key + "_ids"], fixture[key + "_sizes"]
    if not first and ids8.shape[0] == NUM_QUERIES:
        ids8 = ids8.copy(); sizes = sizes.copy()
        ids8[PAGED] = ids8[PAGED_FROM:PAGED_FROM + (PAGED.stop - PAGED.start)]; sizes[PAGED] = sizes[PAGED_FROM:PAGED_FROM + (PAGED.stop - PAGED.start)]
    return np.ascontiguousarray(ids8[:, :k]).astype(np.int32), np.minimum(sizes, k + 1).astype(np.int32)


# ---- (d) the lattice scene -----------------------------------------------------------------------------------------------------------------------

def _small_lattice(seed: int, count: int, base: int, off: int) -> np.ndarray:
    """(count, 3, 3) integer vertices: a base point in [-base, base]^3 plus offsets in [-off, off], non-zero normal"""
    b = _lattice_coords(seed, 2 * count, 3, -base, base)
    o = _lattice_coords(seed + 1, 2 * count, 9, -off, off).reshape(-1, 3, 3)
    P = b[:, None, :] + o
    P = P[(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) != 0).any(axis=1)][:count]
    assert P.shape[0] == count
    return P


def lattice_scene():
    """(tris, queries, P_tris, P_queries): 4000 small lattice triangles (an integer base point in [-14, 14]^3 plus integer offsets in [-2, 2]) and 1024
    lattice queries (half of that kind, half with a base point in [-10, 10]^3 and offsets in [-6, 6]); every coordinate an integer |c| <= 16"""
    Pt = _small_lattice(SEED + 200, LATTICE_TRIS, 14, 2)
    Pq = np.concatenate([_small_lattice(SEED + 202, LATTICE_QUERIES // 2, 14, 2), _small_lattice(SEED + 204, LATTICE_QUERIES // 2, 10, 6)])
    return _tris_of(Pt), _tris_of(Pq), Pt, Pq


def lattice_scene_truth(Pt: np.ndarray, Pq: np.ndarray):
    """(ids (n, 8), sizes) by the exact test alone (pairs whose integer bounding boxes miss each other share no point)"""
    tlo, thi = Pt.min(axis=1), Pt.max(axis=1)
    ids = np.full((Pq.shape[0], KMAX), -1, dtype=np.int32); sizes = np.zeros(Pq.shape[0], dtype=np.int64)
    T = [[tuple(int(c) for c in v) for v in p] for p in Pt]
    for i, p in enumerate(Pq):
        A = [tuple(int(c) for c in v) for v in p]
        near = np.flatnonzero(((tlo <= p.max(axis=0)) & (thi >= p.min(axis=0))).all(axis=1))
        members = [int(j) for j in near if exact_meet(A, T[j])]
        sizes[i] = len(members)
        ids[i, :min(KMAX, len(members))] = members[:KMAX]
    return ids, sizes


# ---- tests/cpp/overlap_tris_host.cpp --------------------------------------------------------------------------------------------------------------

def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("overlap_tris_host", directory, sanitize)


_put = _host.put
_EMPTY = np.zeros(0, dtype=np.int32)


def host_pairs(exe: str, directory, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """triangle a[i] against triangle b[i] through tri_meets of include/hagrid/tri_tri.h"""
    d = str(directory)
    par = os.path.join(d, "tt_pairs_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<i", a.shape[0]))
    out = os.path.join(d, "tt_pairs_out.bin")
    subprocess.run([exe, "pairs", par, _put(d, "tt_pairs_a", a.astype(np.float32)), _put(d, "tt_pairs_b", b.astype(np.float32)), out], check=True, timeout=600)
    return np.fromfile(out, dtype=np.int32) != 0


def _batch_files(d, queries, first, query_labels, tri_labels):
    return [_put(d, "tt_queries", np.ascontiguousarray(queries, dtype=np.float32)), _put(d, "tt_first", _EMPTY if first is None else np.asarray(first, np.int32)),
            _put(d, "tt_qlabels", _EMPTY if query_labels is None else np.asarray(query_labels, np.int32)),
            _put(d, "tt_tlabels", _EMPTY if tri_labels is None else np.asarray(tri_labels, np.int32))]


def host_brute(exe: str, directory, tris, queries, k: int, first=None, query_labels=None, tri_labels=None, any_: bool = False, grid=None):
    """tris_brute_force of include/hagrid/overlap.h over the grid box `grid` = (min, max) (None: scene.grid_box(tris)): (ids (n, k), counts)"""
    d = str(directory)
    n = queries.shape[0]
    glo, ghi = scene.grid_box(tris) if grid is None else grid
    par = os.path.join(d, "tt_brute_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<3i3f3f", n, k, 1 if any_ else 0, *[float(v) for v in glo], *[float(v) for v in ghi]))
    ids, counts = os.path.join(d, "tt_brute_ids.bin"), os.path.join(d, "tt_brute_counts.bin")
    subprocess.run([exe, "brute", par, _put(d, "tt_tris", np.ascontiguousarray(tris, dtype=np.float32)), *_batch_files(d, queries, first, query_labels, tri_labels), ids, counts],
                   check=True, timeout=1200)
    return np.fromfile(ids, dtype=np.int32).reshape(n, k), np.fromfile(counts, dtype=np.int32)


def host_walk(exe: str, directory, grid: dict, tris, queries, k: int, first=None, query_labels=None, tri_labels=None, any_: bool = False):
    """tris_query of include/hagrid/overlap.h over grid arrays (what api.Grid.download returns): (ids (n, k), counts, per-query totals (n, 3) int32: cells
    visited, pairs offered to tri_meets, sub-blocks pruned)"""
    d = str(directory)
    n = queries.shape[0]
    par = os.path.join(d, "tt_walk_params.bin")
    with open(par, "wb") as f:
        f.write(_host.grid_header(grid) + struct.pack("<3i", n, k, 1 if any_ else 0))
    ids, counts, totals = os.path.join(d, "tt_walk_ids.bin"), os.path.join(d, "tt_walk_counts.bin"), os.path.join(d, "tt_walk_totals.bin")
    subprocess.run([exe, "walk", par, *_host.grid_files(d, grid, "tt_"), _put(d, "tt_tris", np.ascontiguousarray(tris, dtype=np.float32)),
                    *_batch_files(d, queries, first, query_labels, tri_labels), ids, counts, totals], check=True, timeout=1200)
    return np.fromfile(ids, dtype=np.int32).reshape(n, k), np.fromfile(counts, dtype=np.int32), np.fromfile(totals, dtype=np.int32).reshape(n, 3)


assert_answers_equal = V.assert_answers_equal
