"""What the capsule-query tests and the fixture generator (tests/golden/make_golden_segments.py) share: the segments of the fixture
tests/golden/segments.npz (regenerated, not stored: counter-based generators of hagrid_amd/scene.py), the host program tests/cpp/segments_host.cpp as
callables (seg_tri pair by pair, the brute-force definition, the walk over grid arrays, with cursors and labels), and the label case.  Scenes are those
of _closest; paging and list comparison are those of _nearest_k."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _closest as K
import _host
import _nearest_k as NK
from _host import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "segments.npz")
ENTRY = scene.NEAREST_ENTRY_DTYPE
RECORD = scene.SEGMENT_RECORD_DTYPE
KMAX = 8
PAGE_K, PAGES = NK.PAGE_K, NK.PAGES
NUM_SEGMENTS = 4096
SEED = 0x7365676D656E74              # "segment"
# the sections of the 4096 segments of a scene
SHORT, OWN, SHORT_R, LONG, AXIS, ZERO, EDGE, PIERCE, OUTSIDE, SPECIAL = (slice(0, 1664), slice(1664, 1920), slice(1920, 2432), slice(2432, 2560), slice(2560, 2752),
                                                                          slice(2752, 3264), slice(3264, 3520), slice(3520, 3776), slice(3776, 4032), slice(4032, 4096))
# the points of _closest.fixture_queries the ZERO section stands on: 192 near the surface, 192 with a radius, 64 on vertices, the 64 special cases
ZERO_POINTS = np.concatenate([np.arange(K.NEAR.start, K.NEAR.start + 192), np.arange(K.RADIUS.start, K.RADIUS.start + 192),
                              np.arange(K.VERTEX.start, K.VERTEX.start + 64), np.arange(K.SPECIAL.start, K.SPECIAL.stop)])


def _rows(*slices):
    return np.concatenate([np.arange(s.start, s.stop) for s in slices])


# the segments with a finite radius: the fixture stores their first three pages at k = 3, and the tests page them to their end (the zero-length ones among
# them: RADIUS points and the r = 0 specials; the labelled OWN section at the end)
STORED = np.concatenate([_rows(SHORT_R), np.arange(LONG.start + 1, LONG.stop, 2), np.arange(ZERO.start + 192, ZERO.start + 384),
                         np.arange(EDGE.start + 1, EDGE.stop, 2), np.arange(SPECIAL.start, SPECIAL.start + 16), _rows(OWN)])
PAGED = STORED
REST = np.setdiff1d(np.arange(NUM_SEGMENTS), STORED)
# the slice of every section the numpy statement is run on in the tests (the generator runs it on all): every 16th segment, and every special one
SAMPLE = np.unique(np.concatenate([np.arange(0, NUM_SEGMENTS, 16), _rows(SPECIAL)]))


def fixture_labels(name: str, tris: np.ndarray):
    """(triangle labels (N, 3), the OWN section's vertex pairs (256, 2)): the mesh's index triples and 256 of its unique edges, spread over the mesh; the
    soup has no shared vertices: triangle j carries 3j, 3j + 1, 3j + 2 and the OWN edges are v0 -> v1 of 256 triangles"""
    if name == "mesh":
        F = np.ascontiguousarray(scene.make_stadium_mesh(0.05)[1], np.int32)
        E = scene.mesh_edges(F)
        return F, np.ascontiguousarray(E[::E.shape[0] // 256][:256])
    tl = np.arange(3 * tris.shape[0], dtype=np.int32).reshape(-1, 3)
    j = np.arange(256) * (tris.shape[0] // 256)
    return tl, np.ascontiguousarray(tl[j][:, 0:2])


def fixture_query_labels(own_pairs: np.ndarray) -> np.ndarray:
    """the (4096, 2) labels of a scene's segments: the OWN section's vertex pairs, -1 (skips nothing) everywhere else"""
    ql = np.full((NUM_SEGMENTS, 2), -1, dtype=np.int32)
    ql[OWN] = own_pairs
    return ql


def fixture_segments(tris: np.ndarray, name: str) -> np.ndarray:
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    inf = np.float32(np.inf)
    s = np.zeros((NUM_SEGMENTS, 8), dtype=np.float32)
    s[SHORT] = scene.make_segments_short(tris, lo, hi, 1664, SEED + 1)
    _, own = fixture_labels(name, tris)
    if name == "mesh":
        V = np.ascontiguousarray(scene.make_stadium_mesh(0.05)[0], np.float32)
        s[OWN] = scene.make_segments(V[own[:, 0]], V[own[:, 1]], np.float32(0.02) * diag)
    else:
        t = tris[own[:, 0] // 3]
        s[OWN] = scene.make_segments(t[:, 0:3], t[:, 0:3] - t[:, 4:7], np.float32(0.02) * diag)
    s[SHORT_R] = s[0:512]; s[SHORT_R, 3] = np.float32(0.02) * diag; s[SHORT_R.start + 256:SHORT_R.stop, 3] = np.float32(0.005) * diag
    s[LONG] = scene.make_segments_diagonal(lo, hi, 128, SEED + 2); s[LONG.start + 1:LONG.stop:2, 3] = np.float32(0.02) * diag
    s[AXIS] = scene.make_segments_axis(lo, hi, 192, SEED + 3)
    p = K.fixture_queries(tris)[ZERO_POINTS]
    s[ZERO, 0:4] = p; s[ZERO, 4:7] = p[:, 0:3]
    s[EDGE] = scene.make_segments_on_edges(tris, 256, SEED + 4); s[EDGE.start + 1:EDGE.stop:2, 3] = np.float32(0.01) * diag
    s[PIERCE] = scene.make_segments_piercing(tris, lo, hi, 256, SEED + 5)
    s[OUTSIDE] = scene.make_segments_outside(lo, hi, 256, SEED + 6)
    sp = scene.make_segments_short(tris, lo, hi, 64, SEED + 7)
    e = scene.make_segments_on_edges(tris, 24, SEED + 8)[0::3]                # the edge itself
    sp[0:8] = e; sp[0:16, 3] = 0.0
    sp[16:24, 3] = np.float32([-1.0, -0.5, -1e-30, -np.inf, -2.0, -1.0, -3.0, -1.0])
    sp[np.arange(24, 32), np.array([0, 1, 2, 4, 5, 6, 0, 5])] = np.float32(np.nan)
    sp[np.arange(32, 40), np.array([0, 1, 2, 4, 5, 6, 4, 1])] = np.float32([inf, -inf, inf, -inf, inf, -inf, inf, -inf])
    sp[40:48, 3] = np.float32(np.nan)
    sp[48:56, 4:7] = sp[48:56, 0:3] + (sp[48:56, 4:7] - sp[48:56, 0:3]) * np.float32(1e5)
    sp[56:64, 4:7] = sp[56:64, 0:3] + (sp[56:64, 4:7] - sp[56:64, 0:3]) * np.float32(1e-28)
    s[SPECIAL] = sp
    return s


def edge_labels_case(stride: int = 7):
    """the label case: the stadium mesh at 0.05, every stride-th of its own unique edges as segments (r = 2 % of the diagonal), labels = the edge's two
    vertex indices, triangle labels = the index triples: (tris, faces, segments, labels (n, 2))"""
    V, F = scene.make_stadium_mesh(0.05)
    V = np.ascontiguousarray(V, np.float32); F = np.ascontiguousarray(F, np.int32)
    tris = scene.tris_from_mesh(V, F)
    lo, hi = scene.tris_bbox(tris)
    E = scene.mesh_edges(F)[::stride]
    return tris, F, scene.make_segments(V[E[:, 0]], V[E[:, 1]], np.float32(0.02) * scene.bbox_diagonal(lo, hi)), np.ascontiguousarray(E)


def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("segments_host", directory, sanitize)


def host_pairs(exe: str, directory, tris, segments) -> dict:
    """triangle i against segment i through seg_tri / tri_side of include/hagrid/capsule.h"""
    d = str(directory); n = tris.shape[0]
    par = os.path.join(d, "sg_pairs_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<i", n))
    out = os.path.join(d, "sg_pairs_out.bin")
    subprocess.run([exe, "pairs", par, _host.put(d, "sg_pairs_tris", np.ascontiguousarray(tris, dtype=np.float32)),
                    _host.put(d, "sg_pairs_segments", np.ascontiguousarray(segments, dtype=np.float32)), out], check=True, timeout=600)
    w = np.fromfile(out, dtype=np.uint32).reshape(n, 8)
    return {"valid": w[:, 0] != 0, "d2": w[:, 1].view(np.float32), "q": np.ascontiguousarray(w[:, 2:5]).view(np.float32), "feature": w[:, 5].view(np.int32),
            "side": w[:, 6].view(np.int32), "s": w[:, 7].view(np.float32)}


def host_brute(exe: str, directory, tris, segments, k: int, cursors=None, query_labels=None, tri_labels=None):
    """brute_force of include/hagrid/capsule.h: (entries (n, k), records (n, k))"""
    return NK.host_brute(exe, directory, tris, segments, k, cursors, query_labels, tri_labels, prefix="sg_", record=RECORD, extra=struct.pack("<i", 0))


def host_walk(exe: str, directory, grid: dict, tris, segments, k: int, cursors=None, query_labels=None, tri_labels=None, box_only=False):
    """segment_query of include/hagrid/capsule.h over grid arrays (what api.Grid.download returns): (entries (n, k), records (n, k), per-query counts
    (n, 4) int32: cells visited, triangles tested, pruned, list full).  box_only: the lower bound without its separating axes"""
    return NK.host_walk(exe, directory, grid, tris, segments, k, cursors, query_labels, tri_labels, prefix="sg_", record=RECORD,
                        extra=struct.pack("<i", 1 if box_only else 0))


def pack_lists(entries, pages) -> dict:
    """how the fixture holds one scene: a STORED segment's k = 8 list and its three pages side by side (a page repeats what the list holds, and side by side
    the file's compression sees it), the k = 8 lists of the other segments apart; ids and the bits of d2"""
    pq = np.transpose(pages, (1, 0, 2)).reshape(STORED.size, PAGES * PAGE_K)
    both = np.concatenate([entries[STORED], pq], axis=1)
    return {"_stored_id": both["id"].astype(np.int32), "_stored_d2": np.ascontiguousarray(both["d2"]).view(np.uint32),
            "_rest_id": entries[REST]["id"].astype(np.int32), "_rest_d2": np.ascontiguousarray(entries[REST]["d2"]).view(np.uint32)}


def fixture_lists(fixture, name: str):
    """(entries (4096, 8) of one scene of the fixture, its pages (PAGES, len(STORED), PAGE_K))"""
    both = NK.entries_of(fixture[name + "_stored_d2"].view(np.float32), fixture[name + "_stored_id"])
    e = np.zeros((NUM_SEGMENTS, KMAX), dtype=ENTRY)
    e[STORED] = both[:, :KMAX]
    e[REST] = NK.entries_of(fixture[name + "_rest_d2"].view(np.float32), fixture[name + "_rest_id"])
    pages = np.ascontiguousarray(np.transpose(both[:, KMAX:].reshape(STORED.size, PAGES, PAGE_K), (1, 0, 2)))
    return e, pages


# ---- exact arithmetic: the distance between a segment and a triangle in rationals, written independently of capsule.h -----------------

def _F3(v):
    from fractions import Fraction
    return tuple(Fraction(int(x)) for x in v)


def _fsub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def _fdot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _fcross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def _fat(a, d, t): return (a[0] + d[0] * t, a[1] + d[1] * t, a[2] + d[2] * t)


def exact_point_seg(p, a, b):
    ab = _fsub(b, a); L = _fdot(ab, ab)
    t = 0 if L == 0 else min(max(_fdot(_fsub(p, a), ab) / L, 0), 1)
    w = _fsub(p, _fat(a, ab, t))
    return _fdot(w, w)


def exact_point_tri(p, v0, v1, v2):
    best = min(exact_point_seg(p, v0, v1), exact_point_seg(p, v1, v2), exact_point_seg(p, v2, v0))
    n = _fcross(_fsub(v1, v0), _fsub(v2, v0)); nn = _fdot(n, n)
    if nn > 0 and all(_fdot(_fcross(_fsub(y, x), _fsub(p, x)), n) >= 0 for x, y in ((v0, v1), (v1, v2), (v2, v0))):
        h = _fdot(_fsub(p, v0), n)
        best = min(best, h * h / nn)
    return best


def exact_seg_seg(a, b, c, d):
    """the minimum of a convex quadratic over the unit square: its critical point if it lies inside, else on the boundary -- an end against a segment"""
    best = min(exact_point_seg(a, c, d), exact_point_seg(b, c, d), exact_point_seg(c, a, b), exact_point_seg(d, a, b))
    u = _fsub(b, a); v = _fsub(d, c); w = _fsub(a, c)
    A, B, E = _fdot(u, u), _fdot(u, v), _fdot(v, v)
    den = A * E - B * B
    if den != 0:
        s = (B * _fdot(v, w) - E * _fdot(u, w)) / den
        t = (A * _fdot(v, w) - B * _fdot(u, w)) / den
        if 0 <= s <= 1 and 0 <= t <= 1:
            x = _fsub(_fat(a, u, s), _fat(c, v, t))
            best = min(best, _fdot(x, x))
    return best


def exact_seg_tri(a, b, v0, v1, v2):
    best = min(exact_point_tri(a, v0, v1, v2), exact_point_tri(b, v0, v1, v2), exact_seg_seg(a, b, v0, v1), exact_seg_seg(a, b, v1, v2), exact_seg_seg(a, b, v2, v0))
    n = _fcross(_fsub(v1, v0), _fsub(v2, v0))
    ha, hb = _fdot(_fsub(a, v0), n), _fdot(_fsub(b, v0), n)
    if ha * hb < 0:
        x = _fat(a, _fsub(b, a), ha / (ha - hb))
        if all(_fdot(_fcross(_fsub(q, p), _fsub(x, p)), n) >= 0 for p, q in ((v0, v1), (v1, v2), (v2, v0))):
            best = 0
    return best


def exact_family(per_class: int = 100, seed: int = 20240611):
    """(v0, v1, v2, a, b): integer arrays (5 * per_class, 3), |c| <= 64, triangles with area: segments that CROSS the face (through an interior lattice
    combination), TOUCH it at a vertex (an end on a vertex, or passing through one), run PARALLEL to an edge, lie COPLANAR with the face, and SKEW ones"""
    rng = np.random.default_rng(seed)
    out = []
    for cls in range(5):
        got = 0
        while got < per_class:
            v0, v1, v2 = (rng.integers(-32, 33, 3) for _ in range(3))
            e1, e2 = v1 - v0, v2 - v0
            n = np.cross(e1, e2)
            if not n.any():
                continue
            if cls == 0:                                    # crossing: through v0 + (e1 + e2) / 4 scaled to the lattice, along a random direction
                m = 4 * v0 + e1 + e2
                w = rng.integers(-6, 7, 3)
                if not w.any() or np.dot(w, n) == 0 or m[0] % 4 or m[1] % 4 or m[2] % 4:
                    continue
                a, b = m // 4 + w * int(rng.integers(1, 4)), m // 4 - w * int(rng.integers(1, 4))
            elif cls == 1:                                  # touching at a vertex
                v = (v0, v1, v2)[int(rng.integers(0, 3))]
                w = rng.integers(-20, 21, 3)
                a, b = (v, v + w) if got % 2 else (v - w, v + w)
            elif cls == 2:                                  # parallel to an edge, off it by a lattice vector
                e = (e1, v2 - v1, e2)[int(rng.integers(0, 3))]
                o = v0 + rng.integers(-12, 13, 3)
                a, b = o, o + e * (1 if got % 2 else -1)
            elif cls == 3:                                  # coplanar: two lattice combinations of the edges
                ca, cb = rng.integers(-1, 3, 2), rng.integers(-1, 3, 2)
                a, b = v0 + ca[0] * e1 + ca[1] * e2, v0 + cb[0] * e1 + cb[1] * e2
            else:
                a, b = rng.integers(-64, 65, 3), rng.integers(-64, 65, 3)
            if max(np.abs(a).max(), np.abs(b).max()) > 64:
                continue
            out.append((v0, v1, v2, a, b)); got += 1
    return tuple(np.array([o[i] for o in out], dtype=np.int64) for i in range(5))
