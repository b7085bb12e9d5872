"""What the oriented-box tests and the fixture generator (tests/golden/make_golden_obb.py) share: the exact box / triangle test in rational arithmetic that
is the yardstick, the pairs, scenes and queries of the fixture tests/golden/obb.npz (regenerated, not stored: counter-based generators of
hagrid_amd/scene.py) and the host program tests/cpp/obb_host.cpp as callables."""
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np

from hagrid_amd import scene

import _host
import _overlap as V
import _overlap_tris as W
from _host import ROOT, INC, oracle_grid, oracle_grid_arrays                # names the tests use

FIXTURE = os.path.join(ROOT, "tests", "golden", "obb.npz")
SCENES = V.SCENES
KMAX = 8
KS = (1, 2, 3, 5, 8)
SEED = 0x6F626F78                        # "obox"
NUM_LATTICE_PAIRS = 16384                # an eighth touch at a face, an edge or a vertex of the box
NUM_SCENE_PAIRS = 1024
NUM_QUERIES = 4096
BODY = 32                                # triangles per body: triangle j carries the labels (j // BODY, -1, -1)
# the sections of the 4096 queries of a scene
SMALL, BIG, OWN, PLANK, SHEAR, FLAT, OUTSIDE, FAR, BAD, PAGED = (slice(0, 1536), slice(1536, 2048), slice(2048, 2816), slice(2816, 2944), slice(2944, 3200),
                                                                 slice(3200, 3456), slice(3456, 3712), slice(3712, 3840), slice(3840, 3968), slice(3968, 4096))
PAGED_FROM = BIG.start                   # query PAGED.start + i repeats query PAGED_FROM + i with first = (third id of that query's answer) + 1
LATTICE_TRIS, LATTICE_QUERIES = 4000, 512

_u = scene._uniform_rows
make_tris = V.make_tris
array_sum = W.array_sum
assert_answers_equal = V.assert_answers_equal


# ---- the yardstick: exact arithmetic, another algorithm -- a vertex inside the box, a triangle edge against a box face, a box edge against the triangle ----

def _add(a, b): return (a[0] + b[0], a[1] + b[1], a[2] + b[2])
def _neg(a): return (-a[0], -a[1], -a[2])


def exact_meet(c, u, v, w, T) -> bool:
    """do the closed box {c + a u + b v + g w : |a|, |b|, |g| <= 1} (with volume) and the closed triangle T (three vertices, not degenerate) share a
    point?  Exact for int and Fraction coordinates.  Two convex bodies of which one has volume and the other is flat meet exactly when a vertex of the
    triangle lies in the box, or an edge of the triangle meets a face of the box, or an edge of the box meets the triangle."""
    sub, dot, cross = W._sub, W._dot, W._cross
    det = dot(u, cross(v, w))
    assert det != 0, "the exact test is for boxes with volume"
    n0, n1, n2 = cross(v, w), cross(w, u), cross(u, v)
    for p in T:                                             # Cramer: p - c = a u + b v + g w
        d = sub(p, c)
        if abs(dot(d, n0)) <= abs(det) and abs(dot(d, n1)) <= abs(det) and abs(dot(d, n2)) <= abs(det):
            return True
    ax = (u, v, w)
    for i in range(3):
        a, b1, b2 = ax[i], ax[(i + 1) % 3], ax[(i + 2) % 3]
        for s in (a, _neg(a)):
            m = _add(c, s)
            q = [_add(m, _add(_neg(b1), _neg(b2))), _add(m, _add(b1, _neg(b2))), _add(m, _add(b1, b2)), _add(m, _add(_neg(b1), b2))]
            for F in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):      # the face as two triangles
                if any(W._segment_meets_tri(T[e], T[(e + 1) % 3], F) for e in range(3)):
                    return True
        for s1 in (b1, _neg(b1)):                           # the four box edges along a
            for s2 in (b2, _neg(b2)):
                m = _add(c, _add(s1, s2))
                if W._segment_meets_tri(_add(m, _neg(a)), _add(m, a), T):
                    return True
    return False


def _rat(x):
    return tuple(Fraction(float(t)) for t in x)


def exact_pairs(obbs: np.ndarray, tris: np.ndarray, grow: float = 0.0) -> np.ndarray:
    """exact_meet of box i and triangle i: the float32 records and vertices read as rationals.  grow: every axis is first made longer (shorter, if
    negative) by that length -- in float64, the result again read as rationals: the box whose faces lie `grow` farther out"""
    O = scene._obb_rows(obbs).astype(np.float64); Vx = scene.tri_vertices(tris)
    if grow:
        for a in (4, 8, 12):
            length = np.sqrt((O[:, a:a + 3] ** 2).sum(axis=1))
            O[:, a:a + 3] *= (1.0 + grow / np.where(length > 0, length, 1.0))[:, None]
    return np.array([exact_meet(_rat(o[0:3]), _rat(o[4:7]), _rat(o[8:11]), _rat(o[12:15]), [_rat(p) for p in t]) for o, t in zip(O, Vx)], dtype=bool)


# ---- (a) lattice pairs: everything in HALF units (integers), |coordinate| <= 16 ---------------------------------------------------------------------

_FRAMES = (((1, 1, 0), (-1, 1, 0), (0, 0, 1)), ((1, 0, 1), (0, 1, 0), (-1, 0, 1)), ((1, 1, 1), (1, -1, 0), (1, 1, -2)), ((2, 1, 0), (-1, 2, 0), (0, 0, 1)),
           ((0, 1, 1), (0, -1, 1), (1, 0, 0)), ((1, 2, 2), (2, 1, -2), (2, -2, 1)))
_PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))


def _ints(seed, count, width, lo, hi):
    return W._lattice_coords(seed, count, width, lo, hi)


def lattice_frames(seed: int, count: int) -> np.ndarray:
    """(count, 3, 3) integer axes u, v, w in half units, every component |.| <= 4, det != 0: a third rotations by multiples of 90 degrees (signed
    permutations of half extents 1 .. 4), a third integer frames such as (1, 1, 0), (-1, 1, 0), (0, 0, 1) (scaled by 1 or 2, axes permuted), a third sheared
    ((a, 0, 0), (s, b, 0), (t, r, c) with the coordinates permuted)"""
    r = _ints(seed, count, 12, 0, 1 << 20)
    A = np.zeros((count, 3, 3), dtype=np.int64)
    for i in range(count):
        kind = i % 3
        perm = _PERMS[r[i, 0] % 6]
        if kind == 0:
            for a in range(3):
                A[i, a, perm[a]] = (1 + r[i, 1 + a] % 4) * (1 if r[i, 4 + a] % 2 else -1)
        elif kind == 1:
            f = np.array(_FRAMES[r[i, 1] % len(_FRAMES)], dtype=np.int64)
            s = 1 + r[i, 2] % 2
            if np.abs(f).max() * s > 4:
                s = 1
            A[i] = (f * s)[list(perm)] * np.array([1 if r[i, 4 + a] % 2 else -1 for a in range(3)])[:, None]
        else:
            a, b, c = (1 + r[i, 1 + j] % 4 for j in range(3))
            s, t, q = (int(r[i, 4 + j] % 5) - 2 for j in range(3))
            M = np.array([[a, 0, 0], [s, b, 0], [t, q, c]], dtype=np.int64)
            A[i] = M[:, list(perm)] * (1 if r[i, 7] % 2 else -1)
    assert (np.abs(A).max() <= 4) and (np.linalg.det(A.astype(np.float64)) != 0).all()
    return A


def lattice_pairs():
    """(obbs, tris, P): 16 384 pairs in half units -- P = (c, u, v, w, t0, t1, t2) as (n, 7, 3) integers, the records and Tri rows in float32 (P / 2).  The
    first eighth TOUCH: a triangle vertex is a face centre, an edge midpoint or a corner of the box and the other two lie beyond a face through it.  Of the
    rest half have vertices within 8 half units of the box centre (contacts are frequent), half anywhere in [-32, 32]."""
    n = NUM_LATTICE_PAIRS
    A = lattice_frames(SEED + 1, n)
    c = _ints(SEED + 2, n, 3, -12, 12)
    touch = n // 8
    P = np.zeros((n, 7, 3), dtype=np.int64)
    P[:, 0] = c; P[:, 1:4] = A
    r = _ints(SEED + 3, n, 12, 0, 1 << 20)
    d = _ints(SEED + 4, n, 6, -4, 4).reshape(n, 2, 3)
    near = _ints(SEED + 5, n, 9, -8, 8).reshape(n, 3, 3)
    wide = _ints(SEED + 6, n, 9, -32, 32).reshape(n, 3, 3)
    for i in range(n):
        if i < touch:
            coef = [0, 0, 0]
            face = r[i, 0] % 3
            coef[face] = 1 if r[i, 1] % 2 else -1
            kind = i % 3                                    # 0: face centre, 1: edge midpoint, 2: corner
            if kind >= 1: coef[(face + 1) % 3] = 1 if r[i, 2] % 2 else -1
            if kind == 2: coef[(face + 2) % 3] = 1 if r[i, 3] % 2 else -1
            p = c[i] + coef[0] * A[i, 0] + coef[1] * A[i, 1] + coef[2] * A[i, 2]
            out = np.cross(A[i, (face + 1) % 3], A[i, (face + 2) % 3])
            if np.dot(out, A[i, face]) * coef[face] < 0:
                out = -out                                  # the outward normal of that face
            T = [p]
            for j in range(2):
                dj = d[i, j].copy()
                if np.dot(out, dj) < 0: dj = -dj
                if np.dot(out, dj) == 0: dj = dj + np.sign(out)         # strictly beyond the face
                T.append(p + dj)
            P[i, 4:7] = T
        else:
            P[i, 4:7] = (c[i] + near[i]) if i % 2 else wide[i]
        k = 0
        while not np.cross(P[i, 5] - P[i, 4], P[i, 6] - P[i, 4]).any():         # a degenerate triangle: move a vertex
            P[i, 6] = P[i, 6] + np.array(((1, 2, 3), (3, 1, 2), (2, 3, 1))[k % 3]) * (1 if P[i, 6].sum() <= 0 else -1); k += 1
    assert np.abs(P).max() <= 32 and np.cross(P[:, 5] - P[:, 4], P[:, 6] - P[:, 4]).any(axis=1).all()
    H = (P.astype(np.float32) * np.float32(0.5)).astype(np.float32)
    return scene.make_obbs(H[:, 0], H[:, 1], H[:, 2], H[:, 3]), scene.tris_from_vertices(H[:, 4], H[:, 5], H[:, 6]), P


def lattice_truth(P: np.ndarray) -> np.ndarray:
    t = lambda x: tuple(int(v) for v in x)
    return np.array([exact_meet(t(p[0]), t(p[1]), t(p[2]), t(p[3]), [t(p[4]), t(p[5]), t(p[6])]) for p in P], dtype=bool)


# ---- (b) queries of a scene -------------------------------------------------------------------------------------------------------------------------

def scene_labels(num_tris: int) -> np.ndarray:
    """(num_tris, 3) int32: body ids -- triangle j carries (j // BODY, -1, -1)"""
    lab = np.full((num_tris, 3), -1, dtype=np.int32)
    lab[:, 0] = np.arange(num_tris) // BODY
    return lab


rotations = scene.make_rotations


def _rotated(centres, R, half) -> np.ndarray:
    """records with the axes R[:, :, a] * half[:, a]"""
    half = np.asarray(half, np.float32)
    return scene.make_obbs(centres, R[:, :, 0] * half[:, 0:1], R[:, :, 1] * half[:, 1:2], R[:, :, 2] * half[:, 2:3])


_unit = scene._unit_rows
plank_records = scene.make_obb_planks


def own_records(tris: np.ndarray, diag) -> np.ndarray:
    """the oriented box of a triangle: the parallelogram of its two edges at v0, 0.1 % of the diagonal thick along its unit normal"""
    Vx = scene.tri_vertices(tris)
    a = (Vx[:, 1] - Vx[:, 0]).astype(np.float32); b = (Vx[:, 2] - Vx[:, 0]).astype(np.float32)
    c = (Vx[:, 0] + (a + b) * np.float32(0.5)).astype(np.float32)
    n = np.cross(a, b).astype(np.float32)
    n[~n.any(axis=1)] = np.float32([0, 0, 1])
    return scene.make_obbs(c, a * np.float32(0.5), b * np.float32(0.5), _unit(n) * (np.float32(0.001) * diag))


def fixture_queries(tris: np.ndarray, paged_ids=None):
    """(records (4096,) OBB_DTYPE, query_labels (4096,) int32) of a scene.  SMALL: rotated boxes of 0.2 % .. 2 % of the diagonal near the surface; BIG: of
    3 % .. 8 %; OWN: the oriented boxes of triangles of the scene, labelled with their body; PLANK: thin diagonal planks; SHEAR: sheared frames; FLAT: one
    axis zero (every eighth two); OUTSIDE: straddling and beyond the faces of the grid; FAR: centres 100 .. 900 diagonals away, half of them with a long axis
    that reaches back into the scene; BAD: a NaN, an inf, huge axes; PAGED: the first 128 of BIG again with first = (paged_ids[i, 2]) + 1.  Labels outside
    OWN are -1."""
    n = tris.shape[0]
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    q = np.zeros(NUM_QUERIES, dtype=scene.OBB_DTYPE)
    lab = np.full(NUM_QUERIES, -1, dtype=np.int32)
    cnt = lambda sec: sec.stop - sec.start

    def half(sec, seed, lo_frac, hi_frac):
        return ((np.float32(lo_frac) + np.float32(hi_frac - lo_frac) * _u(seed, cnt(sec), 3)) * diag).astype(np.float32)
    q[SMALL] = _rotated(scene.make_points_near_surface(tris, lo, hi, cnt(SMALL), SEED + 10), rotations(SEED + 11, cnt(SMALL)), half(SMALL, SEED + 12, 0.002, 0.02))
    q[BIG] = _rotated(V.mixed_centres(tris, lo, hi, cnt(BIG), SEED + 13), rotations(SEED + 15, cnt(BIG)), half(BIG, SEED + 16, 0.03, 0.08))
    own = np.minimum((_u(SEED + 17, cnt(OWN), 1)[:, 0] * np.float32(n)).astype(np.int64), n - 1)
    q[OWN] = own_records(tris[own], diag); lab[OWN] = own // BODY
    q[PLANK] = plank_records(lo, hi, cnt(PLANK), SEED + 18)
    # sheared: a rotated box whose second and third axes lean into the first
    R = rotations(SEED + 19, cnt(SHEAR)); h = half(SHEAR, SEED + 20, 0.005, 0.04); s = np.float32(2.0) * _u(SEED + 21, cnt(SHEAR), 2) - np.float32(1.0)
    u = R[:, :, 0] * h[:, 0:1]
    q[SHEAR] = scene.make_obbs(scene.make_points_near_surface(tris, lo, hi, cnt(SHEAR), SEED + 22), u, R[:, :, 1] * h[:, 1:2] + u * s[:, 0:1], R[:, :, 2] * h[:, 2:3] + u * s[:, 1:2])
    f = _rotated(scene.make_points_near_surface(tris, lo, hi, cnt(FLAT), SEED + 23), rotations(SEED + 24, cnt(FLAT)), half(FLAT, SEED + 25, 0.005, 0.05))
    for i in range(cnt(FLAT)):
        f[i][("u", "v", "w")[i % 3]] = 0
        if i % 8 == 7: f[i][("u", "v", "w")[(i + 1) % 3]] = 0
    q[FLAT] = f
    # outside: centres on and beyond the faces of the scene box
    c = scene.make_points_uniform(lo, hi, cnt(OUTSIDE), SEED + 26, enlarge=0.0)
    i = np.arange(cnt(OUTSIDE)); a = i % 3; up = (i // 3) % 2 == 0
    off = np.where(i % 4 == 0, np.float32(0.0), np.where(i % 4 == 1, np.float32(0.03), np.where(i % 4 == 2, np.float32(0.08), np.float32(0.5)))) * diag
    c[i, a] = np.where(up, hi[a] + off, lo[a] - off)
    q[OUTSIDE] = _rotated(c, rotations(SEED + 27, cnt(OUTSIDE)), half(OUTSIDE, SEED + 28, 0.02, 0.06))
    # far: the float prune's switched-off branch
    d = _unit(np.float32(2.0) * _u(SEED + 29, cnt(FAR), 3) - np.float32(1.0) + np.float32(1e-3))
    dist = ((np.float32(100.0) + np.float32(800.0) * _u(SEED + 30, cnt(FAR), 1)) * diag).astype(np.float32)
    centre = ((lo + hi) * np.float32(0.5)).astype(np.float32)
    far = _rotated((centre + d * dist).astype(np.float32), rotations(SEED + 31, cnt(FAR)), half(FAR, SEED + 32, 0.01, 0.05))
    reach = np.arange(cnt(FAR)) % 2 == 1
    far["u"][reach] = (-d * dist * np.float32(1.001))[reach]            # from the far centre back through the scene
    q[FAR] = far
    bad = _rotated(scene.make_points_near_surface(tris, lo, hi, cnt(BAD), SEED + 33), rotations(SEED + 34, cnt(BAD)), half(BAD, SEED + 35, 0.01, 0.05))
    rows = bad.view(np.float32).reshape(-1, 16)
    cols = (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)
    for i in range(cnt(BAD)):
        col = cols[(i // 4) % 12]
        if i % 4 == 0:   rows[i, col] = np.float32(np.nan)
        elif i % 4 == 1: rows[i, col] = np.float32(np.inf) if (i // 4) % 2 else np.float32(-np.inf)
        elif i % 4 == 2: rows[i, 4 + 4 * ((i // 4) % 3):7 + 4 * ((i // 4) % 3)] *= np.float32(1e30)          # a huge axis: finite, legal
        else:            rows[i, 4:7] = np.float32(3.0e38) * np.sign(rows[i, 4:7])                              # sums overflow
    q[BAD] = bad
    q[PAGED] = q[PAGED_FROM:PAGED_FROM + cnt(PAGED)]
    if paged_ids is not None:
        q["first"][PAGED] = np.asarray(paged_ids)[:, 2].astype(np.int32) + 1
    return q, lab


def scene_queries(fixture, name: str, tris: np.ndarray):
    """the queries of a scene, the paged ones from the fixture's answers; checked against the fixture's checksum"""
    q, lab = fixture_queries(tris, fixture[name + "_ids"][PAGED_FROM:PAGED_FROM + (PAGED.stop - PAGED.start)])
    assert array_sum(q) + array_sum(lab) == int(fixture[name + "_query_sum"]), "the fixture's queries are the generators' queries"
    return q, lab


def expected(fixture, key: str, k: int):
    """(ids (n, k), counts) of the answers `key` for k, from |S| and the first 8 ids"""
    return np.ascontiguousarray(fixture[key + "_ids"][:, :k]).astype(np.int32), np.minimum(fixture[key + "_sizes"], k + 1).astype(np.int32)


def scene_pairs(tris: np.ndarray, q: np.ndarray, seed: int):
    """(1024, 2) int32 pairs (query i, triangle j): queries of SMALL, OWN and SHEAR, up to four triangles each whose bounding box meets the query's"""
    glo, ghi = scene.grid_box(tris)
    B = scene.clip_boxes(scene.obb_boxes(q, glo, ghi), glo, ghi)
    Vx = scene.tri_vertices(tris); tlo = Vx.min(axis=1); thi = Vx.max(axis=1)
    pool = np.concatenate([np.arange(SMALL.start, SMALL.stop), np.arange(OWN.start, OWN.stop), np.arange(SHEAR.start, SHEAR.stop)])
    pick = pool[np.minimum((_u(seed, 4 * NUM_SCENE_PAIRS, 1)[:, 0] * np.float32(pool.size)).astype(np.int64), pool.size - 1)]
    pairs = []
    for i in pick:
        m = ((tlo <= B[i, 4:7]) & (thi >= B[i, 0:3])).all(axis=1)
        for j in np.flatnonzero(m)[:4]:
            pairs.append((i, j))
        if len(pairs) >= NUM_SCENE_PAIRS:
            break
    assert len(pairs) >= NUM_SCENE_PAIRS
    return np.array(pairs[:NUM_SCENE_PAIRS], dtype=np.int32)


def pair_decision(tris, q, pairs) -> np.ndarray:
    """the full pair decision of the query for (i, j): triangle j meets the grown, clipped bounding box of box i AND obb_pairs"""
    glo, ghi = scene.grid_box(tris)
    B = scene.clip_boxes(scene.obb_boxes(q[pairs[:, 0]], glo, ghi), glo, ghi)
    return scene.overlap_pairs(tris[pairs[:, 1]], B) & scene.obb_pairs(tris[pairs[:, 1]], q[pairs[:, 0]])


# ---- (c) the integer lattice scene and axis-aligned records on half-integers ----------------------------------------------------------------------------

def lattice_scene():
    """(tris, records, boxes): the 4000 integer lattice triangles of the contact fixture; 512 axis-aligned records with centres on integers and half
    extents on half-integers (1.5, 2.5 or 3.5), so that every bound lies on a half-integer and nothing touches; and the same boxes as box records"""
    tris = W.lattice_scene()[0]
    c = _ints(SEED + 40, LATTICE_QUERIES, 3, -12, 12).astype(np.float32)
    h = (_ints(SEED + 41, LATTICE_QUERIES, 3, 1, 3).astype(np.float32) + np.float32(0.5)).astype(np.float32)
    z = np.zeros(LATTICE_QUERIES, dtype=np.float32)
    perm = np.arange(LATTICE_QUERIES) % 3                    # which axis of the record lies along x: the order of the axes does not matter
    ax = [np.stack([h[:, 0], z, z], axis=1), np.stack([z, h[:, 1], z], axis=1), np.stack([z, z, h[:, 2]], axis=1)]
    sel = lambda k: np.where((perm == 0)[:, None], ax[k % 3], np.where((perm == 1)[:, None], ax[(k + 1) % 3], ax[(k + 2) % 3]))
    sign = np.where(np.arange(LATTICE_QUERIES) % 2 == 0, np.float32(1.0), np.float32(-1.0))[:, None]
    rec = scene.make_obbs(c, sel(0) * sign, sel(1), sel(2) * sign)
    boxes = np.zeros((LATTICE_QUERIES, 8), dtype=np.float32)
    boxes[:, 0:3] = c - h; boxes[:, 4:7] = c + h
    return tris, rec, boxes


# ---- tests/cpp/obb_host.cpp ------------------------------------------------------------------------------------------------------------------------------

def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("obb_host", directory, sanitize)


_put = _host.put
_EMPTY = np.zeros(0, dtype=np.int32)


def _rows(obbs) -> np.ndarray:
    return scene._obb_rows(obbs)


def host_pairs(exe: str, directory, obbs: np.ndarray, tris: np.ndarray) -> np.ndarray:
    """box i against triangle i through obb_meets of include/hagrid/obb.h"""
    d = str(directory)
    par = os.path.join(d, "ob_pairs_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<i", tris.shape[0]))
    out = os.path.join(d, "ob_pairs_out.bin")
    subprocess.run([exe, "pairs", par, _put(d, "ob_pairs_a", _rows(obbs)), _put(d, "ob_pairs_b", np.ascontiguousarray(tris, dtype=np.float32)), out], check=True, timeout=600)
    return np.fromfile(out, dtype=np.int32) != 0


def _batch_files(d, obbs, query_labels, tri_labels):
    return [_put(d, "ob_obbs", _rows(obbs)), _put(d, "ob_qlabels", _EMPTY if query_labels is None else np.asarray(query_labels, np.int32)),
            _put(d, "ob_tlabels", _EMPTY if tri_labels is None else np.asarray(tri_labels, np.int32))]


def host_brute(exe: str, directory, tris, obbs, k: int, query_labels=None, tri_labels=None, any_: bool = False, grid=None):
    """obb_brute_force of include/hagrid/obb.h over the grid box `grid` = (min, max) (None: scene.grid_box(tris)): (ids (n, k), counts)"""
    d = str(directory)
    n = _rows(obbs).shape[0]
    glo, ghi = scene.grid_box(tris) if grid is None else grid
    par = os.path.join(d, "ob_brute_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<3i3f3f", n, k, 1 if any_ else 0, *[float(v) for v in glo], *[float(v) for v in ghi]))
    ids, counts = os.path.join(d, "ob_brute_ids.bin"), os.path.join(d, "ob_brute_counts.bin")
    subprocess.run([exe, "brute", par, _put(d, "ob_tris", np.ascontiguousarray(tris, dtype=np.float32)), *_batch_files(d, obbs, query_labels, tri_labels), ids, counts],
                   check=True, timeout=1200)
    return np.fromfile(ids, dtype=np.int32).reshape(n, k), np.fromfile(counts, dtype=np.int32)


def host_walk(exe: str, directory, grid: dict, tris, obbs, k: int, query_labels=None, tri_labels=None, any_: bool = False, float_prune: bool = True):
    """obb_query of include/hagrid/obb.h over grid arrays (what api.Grid.download returns): (ids (n, k), counts, per-query totals (n, 3) int32: cells
    visited, pairs offered to obb_meets, blocks pruned).  float_prune False: the integer range prunes alone."""
    d = str(directory)
    n = _rows(obbs).shape[0]
    par = os.path.join(d, "ob_walk_params.bin")
    with open(par, "wb") as f:
        f.write(_host.grid_header(grid) + struct.pack("<4i", n, k, 1 if any_ else 0, 1 if float_prune else 0))
    ids, counts, totals = os.path.join(d, "ob_walk_ids.bin"), os.path.join(d, "ob_walk_counts.bin"), os.path.join(d, "ob_walk_totals.bin")
    subprocess.run([exe, "walk", par, *_host.grid_files(d, grid, "ob_"), _put(d, "ob_tris", np.ascontiguousarray(tris, dtype=np.float32)),
                    *_batch_files(d, obbs, query_labels, tri_labels), ids, counts, totals], check=True, timeout=1200)
    return np.fromfile(ids, dtype=np.int32).reshape(n, k), np.fromfile(counts, dtype=np.int32), np.fromfile(totals, dtype=np.int32).reshape(n, 3)
