"""The distance lattice by scatter, on the CPU (include/hagrid/distance.h; hagrid_amd/scene.py: distance_lattice): the numpy statement against the fixture
tests/golden/distance_lattice.npz; the host program tests/cpp/distance_host.cpp -- the header's definition over all triangles and the header's
sizes -> sums -> tasks -> splat -> finish run sequentially, with 64 voxels per task and with the kernel's, the tasks in both orders -- against the fixture bit for
bit, and once under the sanitizers; exact cases on a lattice whose centres fall on faces, edges and diagonals; lattices whose voxels are an ulp wide; a single
voxel, a flat lattice, a lattice outside the scene, triangles without a surface, centres that overflow."""
import numpy as np
import pytest

import _distance as D
import _fill_lattice as F
from hagrid_amd import scene


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(D.FIXTURE))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("distance_host")
    return D.build_host(d), d


CASES = D.all_cases()
IDS = [c[1] for c in CASES]


@pytest.mark.parametrize("name,key,origin,size,n", CASES, ids=IDS)
def test_numpy_statement_equals_the_fixture(fixture, name, key, origin, size, n):
    tris = D.tris_of(name)
    assert (fixture[key + "_n"] == n).all()
    for b, f in enumerate(D.BAND_FACTORS):
        band = D.band_of(size, f)
        assert band == fixture[key + "_band"][b]
        got = scene.distance_lattice(tris, origin, size, n, band)
        D.assert_records_equal(got, D.fixture_records(fixture, key, b), f"{key} band {f}")
        # it IS closest_points over the centres with r = band
        pts = scene.lattice_centres(origin, size, n); pts["r"] = band
        if got.size <= 2000:
            D.assert_records_equal(got, scene.closest_points(tris, pts), f"{key} band {f}: closest_points")


def test_no_case_is_all_empty_or_trivial(fixture):
    """the shares of voxels that find a triangle: empty and found voxels side by side in most cases, every voxel fought over on the soup"""
    for name, key, origin, size, n in CASES:
        for b in range(2):
            ids = fixture[key + "_id"][b]
            share = (ids >= 0).mean()
            assert share > 0.2, (key, b, share)
            assert fixture[key + "_pairs"][b] >= (ids >= 0).sum()
    assert (fixture["soup_a_id"] >= 0).all() and fixture["soup_a_pairs"][0] > 300 * 1680
    for key in ("boxes_a", "boxes_b", "solids_a", "solids_brick", "mesh_a"):
        assert (fixture[key + "_id"][0] < 0).any() and (fixture[key + "_id"][0] >= 0).any()


@pytest.mark.parametrize("name,key,origin,size,n", CASES, ids=IDS)
def test_host_scatter_and_definition_equal_the_fixture(fixture, host, name, key, origin, size, n):
    """ids, d2 and records (all 32 bytes) of both paths, for T = 64 and the kernel's T, the tasks first to last and last to first; the counts that do not depend on T"""
    exe, d = host
    tris = D.tris_of(name)
    for b, f in enumerate(D.BAND_FACTORS):
        band = D.band_of(size, f)
        want = D.fixture_records(fixture, key, b)
        found = int((want["id"] >= 0).sum())
        got, cnt = D.host_distance(exe, d, tris, origin, size, n, band, "brute")
        D.assert_records_equal(got, want, f"{key} band {f}: the definition")
        assert cnt[2] == fixture[key + "_pairs"][b] and cnt[3] == found
        tasks = {}
        for T in (64, D.TASK_VOXELS):
            for reverse in (False, True):
                got, cnt = D.host_distance(exe, d, tris, origin, size, n, band, "scatter", T, reverse)
                D.assert_records_equal(got, want, f"{key} band {f}: scatter T={T} reverse={reverse}")
                assert cnt[2] == fixture[key + "_pairs"][b] and cnt[3] == found and cnt[1] >= cnt[0] > 0
                tasks[T] = int(cnt[1])
        assert tasks[64] >= tasks[D.TASK_VOXELS]


def test_host_program_under_the_sanitizers(fixture, tmp_path):
    """a stand-alone binary with address and undefined-behaviour sanitizers (float-cast-overflow among them: the casts of the box rule), on boxes_c and mesh_a"""
    exe = D.build_host(tmp_path, sanitize=True)
    for key in ("boxes_c", "mesh_a"):
        tris, origin, size, n = D.case(key)
        for b, f in enumerate(D.BAND_FACTORS):
            band = D.band_of(size, f)
            for op, T in (("brute", 1), ("scatter", 64), ("scatter", D.TASK_VOXELS)):
                got, _ = D.host_distance(exe, tmp_path, tris, origin, size, n, band, op, T, reverse=T == 64)
                D.assert_records_equal(got, D.fixture_records(fixture, key, b), f"{key} band {f} {op} T={T} (sanitized)")
    # overflowing centres and a huge band go through the float -> int casts of the box rule
    tris = D.tris_of("boxes")
    got, _ = D.host_distance(exe, tmp_path, tris, np.float32([3e38, 0.1, 0.1]), np.float32([3e38, 0.2, 0.2]), (3, 2, 2), 0.5, "scatter", 64)
    assert (got["id"] == -1).all()
    got, _ = D.host_distance(exe, tmp_path, tris, np.float32([-1e30, 0.1, 0.1]), np.float32([1e29, 0.2, 0.2]), (20, 2, 2), 3e38, "scatter", 64)
    assert (got["id"] >= 0).all()


def _all_pairs(tris, origin, size, n):
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    P = F.centres(origin, size, n)
    with np.errstate(all="ignore"):
        valid, d2 = scene._point_tri((P[:, 0:1], P[:, 1:2], P[:, 2:3]), [T[None, :, i] for i in range(12)], False)
    return valid, d2


def test_exact_cases_on_faces_edges_and_diagonals(host):
    """boxes_c: centres fall ON faces, edges and the diagonals two triangles of a face share.  band = 0 finds exactly the voxels with d2 = 0, i.e. the centres on the
    boxes' surfaces; every tie goes to the smallest id"""
    exe, d = host
    tris, origin, size, n = D.case("boxes_c")
    assert (origin == np.float32(-0.5625)).all() and (size == np.float32(0.125)).all() and tuple(n) == (28, 16, 16)
    valid, d2 = _all_pairs(tris, origin, size, n)
    assert valid.all()
    _, on = F.boxes_truth(F.centres(origin, size, n))
    assert on.sum() > 500
    for band in (0.0, 0.125, 0.1875, 0.75):
        got, cnt = D.host_distance(exe, d, tris, origin, size, n, band, "scatter")
        D.assert_records_equal(got, scene.distance_lattice(tris, origin, size, n, band), f"boxes_c band {band}")
        r2 = np.float32(band) * np.float32(band)
        within = d2 <= r2
        found = got["id"] >= 0
        assert (found == within.any(axis=1)).all()
        mn = np.where(within, d2, np.float32(np.inf)).min(axis=1)
        ties = within & (d2 == mn[:, None])
        assert (got["id"][found] == ties.argmax(axis=1)[found]).all(), "a tie did not go to the smallest id"
        assert (got["d2"][found] == mn[found]).all() and (got["d2"][~found] == r2).all()
        if band == 0.0:
            assert (found == on).all() and (got["d2"] == 0).all(), "band 0 finds exactly the centres on the surface"
            assert (ties.sum(axis=1)[found] >= 2).any() and (ties.sum(axis=1)[found] >= 4).any(), "centres on shared diagonals and on edges tie"
            assert cnt[2] == within.sum()


# (400 - 1000 voxels along x, so that the face at x = 1 or x = 2.5 lies inside the lattice and the brute force finds 0.7 - 3 % of the voxels)
HOSTILE = (((0.99999, 0.3, 0.3), (1e-7, 0.2, 0.2), (400, 3, 3), 3e-7),
           ((0.999995, 0.3, 0.3), (3e-8, 0.2, 0.2), (1000, 3, 3), 2e-7),
           ((2.4999, 0.3, 0.3), (2e-7, 0.2, 0.2), (600, 3, 3), 1e-6))


@pytest.mark.parametrize("origin,size,n,band", HOSTILE)
def test_voxels_an_ulp_wide(host, origin, size, n, band):
    """voxel edges near one ulp of the coordinates: neighbouring centres collapse to the same float, the box rule's divisions are off by whole voxels.  A guard --
    a float32 rule without margin passes these as well; the proof is the argument in the header.  Against the brute force, which finds 0.7 - 3 % of the voxels."""
    exe, d = host
    tris = D.tris_of("boxes")
    origin, size = np.float32(origin), np.float32(size)
    want, wc = D.host_distance(exe, d, tris, origin, size, n, band, "brute")
    share = (want["id"] >= 0).mean()
    assert 0.007 <= share <= 0.03, share
    D.assert_records_equal(want, scene.distance_lattice(tris, origin, size, n, band), "the definition against numpy")
    centres = F.centres(origin, size, n)
    assert np.unique(centres[:, 0]).size < n[0], "centres were meant to collapse"
    for T in (64, D.TASK_VOXELS):
        got, cnt = D.host_distance(exe, d, tris, origin, size, n, band, "scatter", T, reverse=T == 64)
        D.assert_records_equal(got, want, f"hostile lattice {origin} T={T}")
        assert cnt[2] == wc[2] and cnt[3] == wc[3]


def test_one_voxel_and_a_flat_lattice(host):
    exe, d = host
    for key in ("boxes_one", "boxes_flat"):
        tris, origin, size, n = D.case(key)
        for f in (0.0, 0.5) + D.BAND_FACTORS:
            band = D.band_of(size, f)
            got, _ = D.host_distance(exe, d, tris, origin, size, n, band, "scatter", 64)
            D.assert_records_equal(got, scene.distance_lattice(tris, origin, size, n, band), f"{key} band {f}")
    tris, origin, size, n = D.case("boxes_one")
    assert tuple(n) == (1, 1, 1) and scene.distance_lattice(tris, origin, size, n, 0.6)["id"][0] >= 0 and scene.distance_lattice(tris, origin, size, n, 0.4)["id"][0] == -1


def test_a_lattice_outside_the_scene(host):
    """all -1, d2 = band * band, q = the centre; no triangle has a voxel box"""
    exe, d = host
    tris = D.tris_of("boxes")
    origin, size, n = np.float32([10.0, -7.0, 3.0]), np.float32([0.25, 0.5, 0.125]), (9, 5, 7)
    band = np.float32(0.7)
    got, cnt = D.host_distance(exe, d, tris, origin, size, n, band, "scatter")
    assert (got["id"] == -1).all() and (got["d2"] == band * band).all() and (got["q"] == F.centres(origin, size, n)).all()
    assert (got["feature"] == 0).all() and (got["side"] == 0).all() and cnt.tolist() == [0, 0, 0, 0]
    D.assert_records_equal(got, scene.distance_lattice(tris, origin, size, n, band), "outside")


def test_triangles_without_a_surface_never_win(host):
    """zero-normal triangles mixed in -- copies of real ones and points ON voxel centres, which would have d2 = 0: they take no part and have no voxel box"""
    exe, d = host
    base, origin, size, n = D.case("boxes_a")
    P = F.centres(origin, size, n)
    ghosts = base.copy(); ghosts[:, 3] = 0; ghosts[:, 7] = 0; ghosts[:, 11] = 0
    points = np.zeros((8, 12), np.float32); points[:, 0:3] = P[::113][:8]
    tris = np.ascontiguousarray(np.concatenate([ghosts[:5], points, base, ghosts[5:]]))
    first = 13
    for f in D.BAND_FACTORS:
        band = D.band_of(size, f)
        want = scene.distance_lattice(base, origin, size, n, band)
        got, cnt = D.host_distance(exe, d, tris, origin, size, n, band, "scatter", 64)
        assert (got["id"][got["id"] >= 0] >= first).all() and (got["id"][got["id"] >= 0] < first + base.shape[0]).all()
        moved = got.copy(); moved["id"] = np.where(got["id"] >= 0, got["id"] - first, -1)
        D.assert_records_equal(moved, want, f"band {f}: the scene without the ghosts")
        D.assert_records_equal(got, scene.distance_lattice(tris, origin, size, n, band), f"band {f}: numpy over the same triangles")
        assert cnt[0] == base.shape[0]


def test_centres_that_overflow_find_nothing(host):
    exe, d = host
    tris = D.tris_of("boxes")
    origin, size, n = np.float32([3e38, 0.1, 0.1]), np.float32([3e38, 0.2, 0.2]), (3, 2, 2)
    with np.errstate(all="ignore"):
        want = scene.distance_lattice(tris, origin, size, n, 0.5)
    assert np.isinf(want["q"][:, 0]).all() and (want["id"] == -1).all()
    for T in (64, D.TASK_VOXELS):
        got, _ = D.host_distance(exe, d, tris, origin, size, n, 0.5, "scatter", T)
        D.assert_records_equal(got, want, "overflowed centres")
