"""Crossing queries, the part that needs no GPU: the fixture tests/golden/crossings.npz (accept and t of every pair by the reference's arithmetic, the
facing by numpy) against hagrid_amd/scene.py and against multi_hit.npz; the host program tests/cpp/crossings_host.cpp -- the brute force and the walk of
include/hagrid/crossings.h, the walk the gfx950 kernel runs -- against the fixture, exactly, for page capacities 1, 2, 3, 4 and 8 over Cell and SmallCell
grids of both expansion modes; hostile rays; the page by itself; the same program under AddressSanitizer and UBSan."""
import subprocess

import numpy as np
import pytest

import _crossings as X
import _multi_hit as M
from hagrid_amd import scene

INC = X.INC


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return np.load(X.FIXTURE)


@pytest.fixture(scope="module")
def scenes():
    return {s: X.make_tris(s) for s in X.SCENES}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("crossings_host")
    return X.build_host(d), d


def test_fixture_shape(fixture, scenes):
    import os
    assert os.path.getsize(X.FIXTURE) < 1000000
    for s in X.SCENES:
        rays, rec = fixture[s + "_rays"], fixture[s + "_records"]
        base = X.base_rays(s, scenes[s])
        assert rays.dtype == np.float32 and rec.dtype == np.uint32 and rec.shape == (rays.shape[0], 4)
        assert (M.bits(rays[:base.shape[0]]) == M.bits(base)).all(), "the fixture's first rays are the generators' rays"
        assert int(fixture[s + "_rays_sum"]) == X.checksum(rays)
        counts = rec[:, 0].view(np.int32)
        assert (np.bincount(counts) == fixture[s + "_hist"]).all()
        assert X.has_paging_coverage(counts, X.COVERED_PAGES[s]), "counts 0, 1, P, P + 1, 2P and beyond: otherwise the paging is not tested"
        assert (rec[counts == 0, 1] == M.bits(rays[counts == 0, 7])).all() and (rec[counts < 2, 2] == 0).all()
    assert fixture["points"].shape == (X.NUM_POINTS, 4) and fixture["point_records"].shape == (X.NUM_POINTS, 3, 4)
    assert fixture["labels"].sum() * 4 >= X.NUM_POINTS, "at least a quarter of the points are inside"


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_fixture_equals_numpy(fixture, scenes, scene_name):
    """scene.ray_crossings, every bit"""
    X.assert_records_equal(scene.ray_crossings(scenes[scene_name], fixture[scene_name + "_rays"]), fixture[scene_name + "_records"], scene_name)


def test_fixture_points_equal_numpy_and_the_labels(fixture, scenes):
    tris, pts = scenes["solids"], fixture["points"]
    tris2, solids = scene.make_closed_solids(X.DETAIL)
    again, labels = X.make_points(tris2, solids)
    assert (M.bits(again) == M.bits(pts)).all() and (labels == fixture["labels"]).all()
    m3 = scene.points_inside(tris, pts)
    X.assert_records_equal(m3["records"], fixture["point_records"].reshape(-1, 4), "points, m = 3")
    assert (m3["inside"] == fixture["inside_m3"]).all()
    assert (fixture["inside_m3"] == fixture["labels"]).all(), "the majority of the three default directions is the analytic label for EVERY point"
    assert (scene.points_inside(tris, pts, winding=True)["inside"] == fixture["inside_m3_winding"]).all()
    assert (scene.points_inside(tris, pts, dirs=scene.CROSSING_DIRS[0:1])["inside"] == fixture["inside_m1"]).all()
    assert (scene.points_inside(tris, pts, dirs=scene.CROSSING_DIRS[0:1], winding=True)["inside"] == fixture["inside_m1_winding"]).all()
    origin, size, n = X.lattice_of(tris)
    assert (M.bits(origin) == M.bits(fixture["lattice_origin"])).all() and (M.bits(size) == M.bits(fixture["lattice_size"])).all()
    assert (scene.points_inside(tris, scene.lattice_centres(origin, size, n))["inside"] == fixture["lattice_inside"]).all()
    assert (fixture["lattice_inside"] == 1).any() and (fixture["lattice_inside"] == 0).any()


@pytest.mark.parametrize("scene_name", M.SCENES)
def test_fixture_agrees_with_multi_hit(fixture, scene_name):
    """min(count, 8) = the number of ids >= 0, t_first = slot 0 bit for bit"""
    mh = np.load(M.FIXTURE)
    n = mh[scene_name + "_rays"].shape[0]
    assert (M.bits(fixture[scene_name + "_rays"][:n]) == M.bits(mh[scene_name + "_rays"])).all()
    rec = fixture[scene_name + "_records"][:n]
    assert (np.minimum(rec[:, 0].view(np.int32), 8) == (mh[scene_name + "_ids"] >= 0).sum(axis=1)).all()
    assert (rec[:, 1] == M.bits(mh[scene_name + "_t"][:, 0])).all()


def test_default_directions():
    d = scene.CROSSING_DIRS.astype(np.float64)
    want = np.array([[3, 1, 2], [-2, 4, 3], [1, -5, 2]], np.float64)
    want /= np.sqrt((want * want).sum(axis=1, keepdims=True))
    assert np.abs(d - want).max() < 1e-7
    assert (scene.CROSSING_DIRS == want.astype(np.float32)).all(), "the literals are the float32 nearest to the exact values"


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_host_brute_force_reproduces_the_fixture(fixture, scenes, host, scene_name):
    exe, d = host
    for paged in (True, False):         # the header's crossings_brute_force, and the same definition by a sort
        got = X.host_query(exe, d, scenes[scene_name], rays=fixture[scene_name + "_rays"], paged=paged)
        X.assert_records_equal(got["records"], fixture[scene_name + "_records"], f"{scene_name} paged={paged}")


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", X.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, scenes, host, scene_name, compress, subset_only):
    """every record equal, no ray excepted, for page capacities 1, 2, 3, 4 and 8; flushes within ceil(m / P) + 1"""
    exe, d = host
    tris = scenes[scene_name]
    G = X.oracle_grid(tris, compress, subset_only)
    assert (G.small_cells is not None) == compress
    arrays = X.oracle_grid_arrays(G)
    rays = fixture[scene_name + "_rays"]
    cells = None
    for page in X.PAGES:
        got = X.host_query(exe, d, tris, grid=arrays, page=page, rays=rays)
        X.assert_records_equal(got["records"], fixture[scene_name + "_records"], f"{scene_name} compress={compress} subset_only={subset_only} P={page}")
        assert got["excess"] <= 0, f"P={page}: a ray flushed {got['excess']} times more than ceil(m / P) + 1"
        assert got["totals"][0] == rays.shape[0] and got["totals"][3] > 0
        assert cells is None or got["totals"][1] == cells, "the cells visited do not depend on the page capacity"
        cells = got["totals"][1]


@pytest.mark.parametrize("compress", [False, True])
def test_host_walk_points_and_lattice(fixture, scenes, host, compress):
    exe, d = host
    tris = scenes["solids"]
    arrays = X.oracle_grid_arrays(X.oracle_grid(tris, compress, True))
    pts = fixture["points"]
    for page in (1, 3, 8):
        got = X.host_query(exe, d, tris, grid=arrays, page=page, points=pts)
        X.assert_records_equal(got["records"], fixture["point_records"].reshape(-1, 4), f"points P={page}")
        assert (got["inside"] == fixture["inside_m3"]).all() and (got["inside"] == fixture["labels"]).all()
        assert got["excess"] <= 0
    for dirs, winding, key in ((None, True, "inside_m3_winding"), (scene.CROSSING_DIRS[0:1], False, "inside_m1"), (scene.CROSSING_DIRS[0:1], True, "inside_m1_winding")):
        assert (X.host_query(exe, d, tris, grid=arrays, page=4, points=pts, dirs=dirs, winding=winding)["inside"] == fixture[key]).all()
        assert (X.host_query(exe, d, tris, points=pts, dirs=dirs, winding=winding, paged=True)["inside"] == fixture[key]).all(), "the header's brute force"
    lattice = (fixture["lattice_origin"], fixture["lattice_size"], fixture["lattice_n"])
    for page in (2, 8):
        assert (X.host_query(exe, d, tris, grid=arrays, page=page, lattice=lattice)["inside"] == fixture["lattice_inside"]).all()
    assert (X.host_query(exe, d, tris, lattice=lattice, paged=True)["inside"] == fixture["lattice_inside"]).all()


def test_inactive_points(scenes, host):
    exe, d = host
    tris = scenes["solids"]
    arrays = X.oracle_grid_arrays(X.oracle_grid(tris, False, True))
    pts = np.zeros((6, 4), np.float32)
    pts[:, 0:3] = (0.3, 0.12, 0.43)              # inside the tube of the first torus
    pts[:, 3] = (np.inf, -1.0, np.nan, 1.0, 0.0, 1e-3)
    pts[3, 0] = np.nan; pts[4, 1] = np.inf
    want = scene.points_inside(tris, pts)
    assert want["inside"].tolist() == [1, -1, -1, -1, -1, 0]
    for grid in (None, arrays):
        got = X.host_query(exe, d, tris, grid=grid, points=pts)
        assert (got["inside"] == want["inside"]).all()
        X.assert_records_equal(got["records"], want["records"], "inactive points")


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", ["soup", "mesh"])
def test_hostile_rays_through_the_host_walk(scenes, host, scene_name, compress):
    """the catalogue of tests/_hostile_rays.py: the expectation is the header's brute force (families (i), (k), (l): X.assert_hostile_records says what holds
    there and why); every inadmissible ray yields the empty record; every ray terminates within the flush bound"""
    import _hostile_rays as H
    exe, d = host
    tris = scenes[scene_name]
    G = X.oracle_grid(tris, compress, True)
    rays, family = H.catalogue(tris, G, mesh=scene_name == "mesh")
    want = X.host_query(exe, d, tris, rays=rays)["records"]
    heavy = np.argsort(-want["id"][:, 0], kind="stable")[:3]            # the header's paged brute force on the rays that cross most (thousands of triangles)
    X.assert_records_equal(X.host_query(exe, d, tris, rays=rays[heavy], paged=True)["records"], want[heavy], "paged brute force, the heaviest rays")
    for page in (1, 8):
        got = X.host_query(exe, d, tris, grid=X.oracle_grid_arrays(G), page=page, rays=rays)
        X.assert_hostile_records(got["records"], want, family, f"P={page}")
        assert got["excess"] <= 0
    refused = ~H._admissible(rays)
    assert refused.any()
    assert (X.rec_bits(want)[refused] == X.empty_records(rays[refused])).all()
    X.assert_records_equal(scene.ray_crossings(tris, rays), want, "numpy on the hostile rays: the brute force in numpy and in the header agree on EVERY family")


def test_page_rules(tmp_path):
    """Page by itself: each triangle once, ties in t by id, a full page drops its last entry, nothing at or before the cursor comes back, pairs straddle pages"""
    src = tmp_path / "page.cpp"
    src.write_text(r'''
#include <cstdio>
#include "hagrid/crossings.h"
using namespace hagrid;
using namespace hagrid::crossings;
int main() {
    Page<4> p; Accum a;
    p.init(3); a.init(9.0f);
    bool r[10];
    r[0] = p.insert(5.0f, 7u << 1);            // [7]
    r[1] = p.insert(5.0f, 7u << 1);            // duplicate
    r[2] = p.insert(5.0f, 3u << 1 | 1u);       // tie in t: id 3 before id 7
    r[3] = p.insert(6.5f, 1u << 1);            // [3, 7, 1], full
    r[4] = p.insert(6.5f, 2u << 1);            // not before (6.5, 1)
    r[5] = p.insert(6.0f, 0u << 1 | 1u);       // before (6.5, 1): [3, 7, 0]
    printf("%d %g\n", int(p.full()), p.last_t);
    p.flush(a);                                 // folds (5,3) (5,7) (6,0); cursor (6, 0)
    printf("%d %d %g %g %g %d\n", a.count, a.winding, a.t_first, a.length, a.pending, int(p.empty()));
    r[6] = p.insert(5.0f, 7u << 1);            // before the cursor
    r[7] = p.insert(6.0f, 0u << 1 | 1u);       // the cursor itself
    r[8] = p.insert(6.5f, 1u << 1);            // after it: the dropped triangle comes back
    r[9] = p.insert(8.5f, 4u << 1);
    p.flush(a);
    for (int i = 0; i < 10; i++) printf("%d", int(r[i]));
    printf("\n%d %d %g %g\n", a.count, a.winding, a.t_first, a.length);
    return 0;
}''')
    exe = str(tmp_path / "page")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC, str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "1 6"
    assert out[1] == "3 -1 5 0 6 1"            # pair (5, 5) adds 0; 6 is pending
    assert out[2] == "1011010011"
    assert out[3] == "5 1 5 0.5"               # the pending 6 pairs with 6.5 across the two pages; 8.5 stays unpaired


def test_host_program_under_sanitizers(fixture, scenes, tmp_path):
    """the host program with -fsanitize=address,undefined, once, as a stand-alone binary on the soup: brute force and walk"""
    exe = X.build_host(tmp_path, sanitize=True)
    tris = scenes["soup"]
    rays = fixture["soup_rays"]
    sel = np.r_[0:256, rays.shape[0] - 64:rays.shape[0]]             # primary rays and the aimed ones with many crossings
    arrays = X.oracle_grid_arrays(X.oracle_grid(tris, True, True))
    got = X.host_query(exe, tmp_path, tris, grid=arrays, page=3, rays=rays[sel])
    X.assert_records_equal(got["records"], fixture["soup_records"][sel], "sanitized walk")
    for paged in (True, False):
        got = X.host_query(exe, tmp_path, tris, rays=rays[sel[-16:]], paged=paged)
        X.assert_records_equal(got["records"], fixture["soup_records"][sel[-16:]], f"sanitized brute force paged={paged}")
