"""Nearest-surface queries, the part that needs no GPU: the per-pair arithmetic of include/hagrid/closest.h (compiled for the host) against its numpy
statement hagrid_amd/scene.py word for word; the numpy statement against an independently written float64 evaluation; the fixture
tests/golden/closest.npz against the statement and against the header's brute force; the host walk tests/cpp/closest_host.cpp -- the walk the gfx950
kernel runs -- over grids of the CPU oracle against the fixture, exactly; the walk's counters; the entry point in header, library and bindings."""
import os
import re
import subprocess

import numpy as np
import pytest

import _closest as K
from hagrid_amd import scene

ROOT = K.ROOT
INC = K.INC

# The column sums of the walk's per-query counters (cells visited, triangles tested, sub-blocks pruned) over the 4096 fixture queries, by (scene, expansion
# mode); Cell and SmallCell grids give the same.  Taken at the parent of the commit that moved the descent into include/hagrid/block_walk.h: the order of
# the visits is part of a counter, so a walk that visits in another order misses these.
WALK_COUNTERS = {("soup", True): (50624, 55458, 453184), ("soup", False): (50606, 55426, 452402),
                 ("mesh", True): (80358, 162644, 1602307), ("mesh", False): (79885, 161857, 1588694)}

# 4 x the largest deviation measured for the operation order of include/hagrid/closest.h on the two fixture scenes (test_statement_against_float64)
TOLERANCE = 4 * 3.76e-8


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return np.load(K.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("closest_host")
    return K.build_host(d), d


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name in K.SCENES:
        tris = K.make_tris(name)
        out[name] = (tris, K.fixture_queries(tris))
    return out


def pair_cases(seed=5):
    """(tris, points): random triangles, slivers, triangles without a surface, and for each kind points in every face / edge / vertex region
    (barycentric coordinates of every sign pattern, in the plane and off it), points on vertices and edges exactly, far points"""
    rng = np.random.default_rng(seed)
    n = 6000
    v0 = rng.uniform(-1, 1, (n, 3)); a = rng.uniform(-0.3, 0.3, (n, 3)); b = rng.uniform(-0.3, 0.3, (n, 3))
    kind = np.arange(n) % 6
    b = np.where((kind == 1)[:, None], a * rng.uniform(0.2, 3.0, (n, 1)) + rng.uniform(-1e-5, 1e-5, (n, 3)), b)      # slivers
    b = np.where((kind == 2)[:, None], a * 2.0, b)                                                                   # collinear: normal 0 or nearly
    a = np.where((kind == 3)[:, None], 0.0, a)                                                                       # an edge of no length
    scale = np.where(kind == 4, 1e-4, 1.0)[:, None]                                                                  # tiny
    a = a * scale; b = b * scale
    offset = np.where(kind == 5, 100.0, 0.0)[:, None]                                                                # far from the origin
    v0 = (v0 + offset).astype(np.float32); v1 = (v0 + a).astype(np.float32); v2 = (v0 + b).astype(np.float32)
    tris = scene.tris_from_vertices(v0, v1, v2)
    tris[kind == 2, 3] = 0; tris[kind == 2, 7] = 0; tris[kind == 2, 11] = 0                                          # ... stored normal exactly 0
    tris[kind == 3, 11] = 1                                                                                         # a record with a normal and an edge of no length: t = 0 / 0
    # barycentric coordinates around and inside the triangle: every sign pattern of (1 - u - v, u, v)
    uv = rng.uniform(-1.5, 2.5, (n, 2))
    h = np.where(rng.random(n) < 0.3, 0.0, rng.normal(0, 0.2, n))[:, None]
    nrm = np.cross(v1 - v0, v2 - v0).astype(np.float64)
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    p = v0 + uv[:, 0:1] * (v1 - v0) + uv[:, 1:2] * (v2 - v0) + h * nrm * np.linalg.norm(v1 - v0, axis=1, keepdims=True)
    p = p.astype(np.float32)
    exact = np.arange(n) % 11
    p = np.where((exact == 0)[:, None], v0, p); p = np.where((exact == 1)[:, None], v1, p); p = np.where((exact == 2)[:, None], v2, p)
    p = np.where((exact == 3)[:, None], (v0 + np.float32(0.5) * (v1 - v0)).astype(np.float32), p)
    p = np.where((exact == 4)[:, None], (p * np.float32(1000.0)).astype(np.float32), p)
    return tris, np.ascontiguousarray(p, np.float32)


def test_pair_arithmetic_header_against_numpy(host):
    """point_tri and tri_side of the header, compiled with g++ -ffp-contract=off, against scene.closest_pairs: valid, feature and side equal, d2 and q
    bit-equal, for every pair"""
    exe, d = host
    tris, pts = pair_cases()
    got = K.host_pairs(exe, d, tris, pts)
    want = scene.closest_pairs(tris, pts)
    assert (got["valid"] == want["valid"]).all()
    v = want["valid"]
    assert (~v).sum() == v.size // 6, "the cases hold triangles without a surface"
    assert (K.bits(got["d2"][v]) == K.bits(want["d2"][v])).all()
    assert (K.bits(got["q"][v]) == K.bits(want["q"][v])).all()
    assert (got["feature"][v] == want["feature"][v]).all() and (got["side"][v] == want["side"][v]).all()
    assert (np.bincount(want["feature"][v], minlength=4) > 200).all(), "every feature occurs"
    assert set(np.unique(want["side"][v])) == {-1, 0, 1}
    assert not np.isnan(want["d2"][v & (np.arange(v.size) % 6 != 3)]).any()


def test_pair_arithmetic_against_float64():
    """the per-pair distance against the float64 evaluation on well-shaped random triangles: a relative 1e-5 and an absolute 1e-6 (coordinates of size 1)"""
    tris, pts = pair_cases(seed=9)
    kind = np.arange(tris.shape[0]) % 6
    ok = (kind == 0) & (np.arange(tris.shape[0]) % 11 != 4)
    want = K.distance_f64(tris[ok], pts[ok], np.arange(ok.sum()))
    got = np.sqrt(scene.closest_pairs(tris[ok], pts[ok])["d2"].astype(np.float64))
    assert np.abs(got - want).max() <= 1e-6 + 1e-5 * want.max()


def test_fixture_is_the_statement(fixture, scenes, host):
    """the stored answers are what scene.closest_points gives (a slice of every section, through numpy) and what the header's brute force gives (all)"""
    exe, d = host
    for name in K.SCENES:
        tris, q = scenes[name]
        assert int(fixture[name + "_query_sum"]) == int(K.bits(q).astype(np.uint64).sum()), "the fixture's queries are the generators' queries"
        want = K.fixture_results(fixture, name)
        K.assert_results_equal(K.host_brute(exe, d, tris, q), want, f"{name}: brute_force of closest.h against the fixture")
        pick = np.concatenate([np.arange(s.start, s.stop)[:48] for s in (K.NEAR, K.UNIFORM, K.RADIUS, K.SURFACE, K.VERTEX)] + [np.arange(K.SPECIAL.start, K.SPECIAL.stop)])
        K.assert_results_equal(scene.closest_points(tris, q[pick]), want[pick], f"{name}: scene.closest_points against the fixture")
    assert os.path.getsize(K.FIXTURE) < 220000


def test_fixture_semantics(fixture, scenes):
    for name in K.SCENES:
        tris, q = scenes[name]
        r = K.fixture_results(fixture, name)
        found = r["id"] >= 0
        r2 = q[:, 3] * q[:, 3]
        assert (r["d2"][found] <= r2[found]).all()
        none = ~found
        assert (r["feature"][none] == 0).all() and (r["side"][none] == 0).all() and (K.bits(r["q"][none]) == K.bits(q[none, 0:3])).all()
        inactive = q[:, 3] < 0
        assert inactive.sum() == 8 and (r["id"][inactive] == -1).all() and (r["d2"][inactive] == -1).all()
        nan = np.isnan(q[:, 0:3]).any(axis=1)
        assert nan.sum() == 8 and (r["id"][nan] == -1).all()
        rest = none & ~inactive & ~nan
        assert (K.bits(r["d2"][rest]) == K.bits(r2[rest])).all()
        assert found[K.NEAR].all() and found[K.UNIFORM].all() and found[K.SURFACE].all() and found[K.VERTEX].all()
        assert 0 < found[K.RADIUS].sum() < 512, "some queries with a radius find nothing"
        sp = K.SPECIAL.start
        assert found[sp:sp + 32].all(), "points outside the grid box find the surface"
        assert found[sp + 32:sp + 40].all() and (r["d2"][sp + 32:sp + 40] == 0).all(), "r = 0 on a vertex finds it at distance 0"
        assert not found[sp + 40:sp + 48].any(), "r = 0 elsewhere finds nothing"
        assert set(np.unique(r["feature"][found])) == {0, 1, 2, 3} and set(np.unique(r["side"][found])) == {-1.0, 0.0, 1.0}
        assert (r["zero"] == 0).all()
        # the triangle named is the one whose per-pair value is stored
        pr = scene.closest_pairs(tris[r["id"][found]], q[found, 0:3])
        assert (K.bits(pr["d2"]) == K.bits(r["d2"][found])).all() and (K.bits(pr["q"]) == K.bits(r["q"][found])).all()


def test_statement_against_float64(fixture, scenes):
    """The float32 answers of the statement against an independently written float64 evaluation (the projection clamped into the triangle region by
    region, not a minimum of candidates), for EVERY query that has a distance.  Unit: the box diagonal, or the query's own distance where that is larger
    (the sixteen far-outside queries: float32 holds a distance to 6e-8 of itself).  MEASURED for this operation order:
        soup: the float32 winner is 0 farther than the float64 one, |sqrt(d2) - distance| <= 3.76e-8  (3.01e-8 without the far-outside queries)
        mesh: the float32 winner is at most 1.66e-9 farther,         |sqrt(d2) - distance| <= 3.32e-8  (2.18e-8 without)
    TOLERANCE = 4 x the largest of them = 1.5e-7.  Ids need not match float64: shared edges and vertices are exact ties.  A query with a radius that found
    nothing has no float64 triangle more than the tolerance inside the radius, and one that found something none more than the tolerance outside."""
    for name in K.SCENES:
        tris, q = scenes[name]
        d = K.deviations_f64(tris, q, K.fixture_results(fixture, name))
        print(name, d)
        assert d["real"] == 4096 - 16 and d["found"] + d["none"] == d["real"], "no query with a distance is left out"
        assert d["excess"] <= TOLERANCE, (name, d)
        assert d["error"] <= TOLERANCE, (name, d)
        assert d["inside"] <= TOLERANCE and d["outside"] <= TOLERANCE, (name, d)


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", K.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, scenes, host, scene_name, compress, subset_only):
    """id, feature and side equal, d2 and q bit-equal, for all 4096 queries, over Cell and SmallCell grids of the CPU oracle, both expansion modes; the
    counters' sums are the pinned ones"""
    exe, d = host
    tris, q = scenes[scene_name]
    G = K.oracle_grid(tris, compress, subset_only)
    assert (G.small_cells is not None) == compress
    got, counts = K.host_walk(exe, d, K.oracle_grid_arrays(G), tris, q)
    K.assert_results_equal(got, K.fixture_results(fixture, scene_name), f"{scene_name} compress={compress} subset_only={subset_only}")
    trivial = (q[:, 3] < 0) | np.isnan(q[:, 0:3]).any(axis=1)
    assert (counts[trivial] == 0).all() and (counts[~trivial, 0] >= 1).all()
    assert tuple(int(v) for v in counts.sum(axis=0, dtype=np.int64)) == WALK_COUNTERS[scene_name, subset_only]


def test_walk_is_no_brute_force(scenes, host):
    """over the near-surface queries of the soup the walk tests fewer than N / 10 triangles per query on average (a guard, not a target; measured: 11.5 of
    20 000), and it does prune"""
    exe, d = host
    tris, q = scenes["soup"]
    G = K.oracle_grid(tris, False, True)
    _, counts = K.host_walk(exe, d, K.oracle_grid_arrays(G), tris, q)
    mean = counts[K.NEAR, 1].mean()
    print("triangles tested per near-surface query:", mean, "cells:", counts[K.NEAR, 0].mean(), "pruned:", counts[K.NEAR, 2].mean())
    assert mean < tris.shape[0] / 10
    assert counts[K.NEAR, 2].sum() > 0


def test_host_walk_under_sanitizers(fixture, scenes, tmp_path):
    """the host program with -fsanitize=address,undefined as a stand-alone binary: the walk (its stack is an array indexed at run time) over a SmallCell grid,
    the first 256 queries of the soup"""
    exe = K.build_host(tmp_path, sanitize=True)
    tris, q = scenes["soup"]
    got, _ = K.host_walk(exe, tmp_path, K.oracle_grid_arrays(K.oracle_grid(tris, True, True)), tris, q[:256])
    K.assert_results_equal(got, K.fixture_results(fixture, "soup")[:256], "sanitized walk")


def test_records_and_entry_point(fixture):
    """the ctypes mirror: record sizes, the symbol declared in the header, exported by the library and bound"""
    from hagrid_amd import api, lib
    assert scene.POINT_QUERY_DTYPE.itemsize == 16 and scene.CLOSEST_DTYPE.itemsize == 32
    assert [scene.CLOSEST_DTYPE.fields[k][1] for k in ("q", "d2", "id", "feature", "side", "zero")] == [0, 12, 16, 20, 24, 28]
    assert api.CLOSEST_DTYPE is scene.CLOSEST_DTYPE and api.POINT_QUERY_DTYPE is scene.POINT_QUERY_DTYPE
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "hagrid_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+hagrid_closest_points\s*\(", code) and re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", code)
    L = lib.load()
    assert "hagrid_closest_points" in lib.SIGNATURES and hasattr(L, "hagrid_closest_points") and len(lib.SIGNATURES["hagrid_closest_points"][1]) == 8
    assert hasattr(api, "closest_points") and "closest_points" in api.__all__
    assert "closest_points" in open(os.path.join(INC, "hagrid", "traverse.h")).read()
    prog = '#include "hagrid_amd.h"\nint main(void) { return sizeof(&hagrid_closest_points) ? 0 : 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-fsyntax-only", "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def header_alone(name):
    return subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC, "-fsyntax-only", "-x", "c++",
                           os.path.join(INC, "hagrid", name)], capture_output=True, text=True)


def test_closest_header_is_cxx11():
    r = header_alone("closest.h")
    assert r.returncode == 0, r.stderr


def test_block_walk_header_is_cxx11():
    r = header_alone("block_walk.h")
    assert r.returncode == 0, r.stderr
