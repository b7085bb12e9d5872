"""The scan-line fill (hagrid_fill_lattice), the part that needs no GPU: the fixture tests/golden/fill_lattice.npz against scene.fill_lattice; the host
program tests/cpp/fill_lattice_host.cpp -- the brute force and the walk of include/hagrid/crossings.h with the row sink, the passes and the workspace byte the
gfx950 kernel runs -- against the fixture, every bit, for page capacities 1, 2, 4 and 8 over Cell and SmallCell grids, every axis mask and both vote rules; what
the inputs must show for the tests to mean something; the truth: the analytic solids, scene.points_inside and the analytic boxes; the sink by itself; the
program under AddressSanitizer and UBSan."""
import os
import subprocess

import numpy as np
import pytest

import _crossings as X
import _fill_lattice as FL
from hagrid_amd import scene

CASES = FL.all_cases()
KEYS = [c[1] for c in CASES]


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return dict(np.load(FL.FIXTURE))


@pytest.fixture(scope="module")
def scenes():
    return {s: FL.make_tris(s) for s in FL.SCENES}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("fill_lattice_host")
    return FL.build_host(d), d


def case_of(key):
    return [c for c in CASES if c[1] == key][0]


def test_fixture_shape(fixture):
    assert os.path.getsize(FL.FIXTURE) < 200000
    assert [tuple(int(v) for v in c[4]) for c in CASES] == [(24, 20, 28), (9, 7, 5), (12, 10, 14), (12, 10, 14), (14, 8, 8), (14, 8, 8), (28, 16, 16), (1, 1, 1), (5, 1, 3),
                                                           (14, 8, 8), (14, 8, 8), (28, 16, 16)]
    for name, key, origin, size, n in CASES:
        assert (fixture[key + "_origin"] == origin).all() and (fixture[key + "_size"] == size).all() and (fixture[key + "_n"] == n).all()
        ins = fixture[key + "_inside"]
        assert ins.dtype == np.int8 and ins.shape == (2, 7, int(np.prod(n))) and ins.min() >= -1 and ins.max() <= 1
        rows = sum(FL.row_counts(n))
        assert fixture[key + "_records"].shape == (rows, 4) and fixture[key + "_abstained"].shape == (2, rows)
    assert any(sum(FL.row_counts(c[4])) % 64 for c in CASES) and FL.row_counts(CASES[0][4]) == (560, 672, 480)


def test_the_inputs_show_what_the_tests_need(fixture, scenes):
    """rows beyond one page, abstaining rows on every axis and voxels at -1 in the soup; none in the solids; the open box abstains"""
    n = fixture["soup_a_n"]
    rc = FL.row_counts(n)
    counts = fixture["soup_a_records"][:, 0].view(np.int32)
    assert counts.max() == 12 and (counts > 8).sum() > 0, "the soup has rows with more than one page of crossings"
    ab = fixture["soup_a_abstained"]
    per_axis = lambda a: [int(a[:rc[0]].sum()), int(a[rc[0]:rc[0] + rc[1]].sum()), int(a[rc[0] + rc[1]:].sum())]
    assert per_axis(ab[0]) == [49, 58, 32] and per_axis(ab[1]) == [83, 101, 67]
    assert (fixture["soup_a_inside"][:, 6] == -1).any(axis=1).all(), "voxels whose three rows all abstain"
    for key in ("solids_a", "solids_brick"):
        assert not fixture[key + "_abstained"].any()
        assert (fixture[key + "_inside"] >= 0).all()
    for key in ("open_box_a", "open_box_b", "open_box_c"):
        assert fixture[key + "_abstained"].any(axis=1).all()
        ins = fixture[key + "_inside"]
        assert any((ins[:, m - 1] == -1).any() for m in (1, 2, 4)), "with one axis an abstaining row leaves its voxels at -1"
        _, on = FL.boxes_truth(FL.centres(*case_of(key)[2:]), FL.BOXES[:1])
        assert (ins[:, 6][:, ~on] >= 0).all(), "with three axes no voxel off the surface is left without a usable row"


@pytest.mark.parametrize("key", KEYS)
def test_fixture_equals_numpy(fixture, scenes, key):
    """scene.fill_lattice, every bit: all three axes and each axis alone, both rules"""
    name, _, origin, size, n = case_of(key)
    for winding in (False, True):
        for mask in (7, 1, 2, 4, 5):
            r = scene.fill_lattice(scenes[name], origin, size, n, axes=mask, winding=winding)
            assert r["inside"].dtype == np.int32 and r["records"].dtype == scene.HIT_DTYPE and r["abstained"].dtype == bool
            FL.assert_fill_equal(r, FL.fixture_case(fixture, key, mask, winding), f"{key} axes={mask} winding={winding}")
    r0 = scene.fill_lattice(scenes[name], origin, size, n, axes=0)
    assert (r0["inside"] == fixture[key + "_inside"][0, 6]).all(), "axes = 0 means 7"


@pytest.mark.parametrize("key", KEYS)
def test_records_are_those_of_the_row_rays(fixture, scenes, key):
    name, _, origin, size, n = case_of(key)
    rays = np.concatenate([scene.lattice_row_rays(origin, size, n, a) for a in range(3)])
    assert rays.shape[0] == sum(FL.row_counts(n)) and (rays[:, 3] == -np.inf).all() and (rays[:, 7] == np.inf).all()
    X.assert_records_equal(scene.ray_crossings(scenes[name], rays), fixture[key + "_records"], key)
    c = FL.centres(origin, size, n).reshape(int(n[2]), int(n[1]), int(n[0]), 3)
    rc = FL.row_counts(n)
    assert (rays[:rc[0], 0:3] == c[:, :, 0].reshape(-1, 3)).all(), "x rows: y fastest"
    assert (rays[rc[0]:rc[0] + rc[1], 0:3] == c[:, 0, :].reshape(-1, 3)).all(), "y rows: x fastest"
    assert (rays[rc[0] + rc[1]:, 0:3] == c[0].reshape(-1, 3)).all(), "z rows: x fastest"


@pytest.mark.parametrize("key", KEYS)
def test_host_brute_force_reproduces_the_fixture(fixture, scenes, host, key):
    exe, d = host
    name, _, origin, size, n = case_of(key)
    for winding in (False, True):
        for mask in FL.MASKS:
            got = FL.host_fill(exe, d, scenes[name], origin, size, n, mask, winding)
            FL.assert_fill_equal(got, FL.fixture_case(fixture, key, mask, winding), f"{key} axes={mask} winding={winding}")
            assert got["totals"][0] == got["abstained"].size and got["totals"][4] == got["abstained"].sum()


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("key", KEYS)
def test_host_walk_reproduces_the_fixture(fixture, scenes, host, key, compress):
    """inside, records and abstaining rows equal for page capacities 1, 2, 4 and 8, every axis mask, both rules; the counters do not depend on the rule"""
    exe, d = host
    name, _, origin, size, n = case_of(key)
    tris = scenes[name]
    G = X.oracle_grid(tris, compress, True)
    assert (G.small_cells is not None) == compress
    arrays = X.oracle_grid_arrays(G)
    for page in FL.PAGES:
        for mask in FL.MASKS:
            totals = []
            for winding in (False, True):
                got = FL.host_fill(exe, d, tris, origin, size, n, mask, winding, grid=arrays, page=page)
                FL.assert_fill_equal(got, FL.fixture_case(fixture, key, mask, winding), f"{key} compress={compress} P={page} axes={mask} winding={winding}")
                totals.append(got["totals"])
            assert (totals[0][:4] == totals[1][:4]).all() and totals[0][0] == FL.rows_of_mask(n, mask).size


def test_truth_on_the_solids(fixture):
    """both rules, every single axis and all three: the analytic inside / outside away from the surfaces, and scene.points_inside on every voxel"""
    tris = FL.make_tris("solids")
    for key, far in (("solids_a", FL.NEAR), ("solids_brick", 0.15 * 0.05)):
        _, _, origin, size, n = case_of(key)
        pts = scene.lattice_centres(origin, size, n)
        truth, dist = FL.solids_truth(pts["p"])
        sel = dist > far
        want = scene.points_inside(tris, pts)["inside"]
        assert (want[sel] == truth[sel]).all()
        if key == "solids_a":
            assert sel.sum() == 12383 and truth[sel].sum() > 50
        else:
            assert truth[0] == 1 and dist[0] > far, "the brick begins inside the sphere"
            assert 0 < truth[sel].sum() < sel.sum()
        for w in (0, 1):
            for mask in (1, 2, 4, 7):
                got = fixture[key + "_inside"][w, mask - 1]
                assert (got[sel] == truth[sel]).all(), f"{key} rule {w} axes {mask}: differs from the analytic solids"
                assert (got == want).all(), f"{key} rule {w} axes {mask}: differs from points_inside"


def test_truth_on_the_boxes(fixture):
    """winding: the analytic boxes on every voxel whose centre is not on a box's closed surface, per axis and for all three; parity is pinned by the fixture and
    is wrong somewhere: rows through the face diagonals and the shared edges"""
    parity_wrong = 0
    for key in ("boxes_a", "boxes_b", "boxes_c", "boxes_one", "boxes_flat"):
        truth, on = FL.boxes_truth(FL.centres(*case_of(key)[2:]))
        assert (~on).any()
        for mask in (1, 2, 4, 7):
            got = fixture[key + "_inside"][1, mask - 1]
            assert (got[~on] == truth[~on]).all(), f"{key} axes {mask}: winding differs from the boxes on {(got[~on] != truth[~on]).sum()} voxels"
            parity_wrong += int((fixture[key + "_inside"][0, mask - 1][~on] != truth[~on]).sum())
    assert fixture["boxes_one_inside"][1, 6][0] == 1 and parity_wrong > 0


def test_row_sink_rules(tmp_path):
    """RowSink by itself: runs between crossings, strict t < tc, the final state, a row that starts inside; combine_votes and the workspace byte"""
    src = tmp_path / "row.cpp"
    src.write_text(r'''
#include <cstdio>
#include "hagrid/crossings.h"
using namespace hagrid;
using namespace hagrid::crossings;
struct Print { void operator()(int first, int stride, int length, int state) const { printf("%d+%dx%d=%d ", first, stride, length, state); } };
int main() {
    RowSink<Print> r;
    r.init(row_of(1, 5, 4, 6, 3), 0.0f, 1.0f, false);       // y row 5 of a 4 x 6 x 3 lattice: x = 1, z = 1, base 25, stride 4, 6 voxels at tc = 0 .. 5
    r(0, -3.0f, 0u); r(1, 0.0f, 2u); r(2, 2.5f, 4u); r(3, 2.75f, 7u); r(4, 9.0f, 9u);
    r.finish();
    printf("| %d\n", r.state());
    RowSink<Print> w;
    w.init(row_of(0, 2, 3, 2, 2), 0.0f, 1.0f, true);
    w(0, 0.5f, 3u); w(1, 0.5f, 5u); w(2, 1.5f, 2u);
    w.finish();
    printf("| %d\n", w.state());
    printf("%d %d %d %d %d\n", combine_votes(0, 0), combine_votes(1, 1), combine_votes(2, 1), combine_votes(3, 2), combine_votes(3, 1));
    unsigned b = row_bits(0xffu, 0, 1, 1); b = row_bits(b, 0, 1, 1) & 3u; b = row_bits(b, 1, 0, 1); b = row_bits(b, 2, 1, 0);
    printf("%u %d %d\n", b, row_answer(b), row_answer(row_bits(b, 2, 0, 0)));
    return 0;
}''')
    exe = str(tmp_path / "row")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", X.INC, str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    # the crossing at t = 0 is NOT before voxel 0 (strict); voxels 1 and 2 lie behind two crossings, voxel 3 .. 5 behind four; five crossings: ends inside
    assert out[0].split() == ["25+4x1=1", "29+4x2=0", "37+4x3=0", "|", "1"]
    assert out[1].split() == ["6+1x1=0", "7+1x1=1", "8+1x1=1", "|", "1"]           # winding -2 behind two entering crossings is inside; -1 at the end: abstains
    assert out[2] == "-1 1 0 1 0"
    assert out[3] == "19 0 1"          # passes 0 and 2 usable, one vote: no majority; without pass 2 the one vote wins


def test_host_program_under_sanitizers(fixture, scenes, tmp_path):
    """the host program with -fsanitize=address,undefined, once, as a stand-alone binary: brute force and walk on the soup (abstaining rows, more than one page)
    and the open box"""
    exe = FL.build_host(tmp_path, sanitize=True)
    for key, compress in (("soup_a", True), ("open_box_b", False)):
        name, _, origin, size, n = case_of(key)
        arrays = X.oracle_grid_arrays(X.oracle_grid(scenes[name], compress, True))
        for mask, winding, page in ((7, False, 3), (2, True, 8), (5, True, 1)):
            want = FL.fixture_case(fixture, key, mask, winding)
            FL.assert_fill_equal(FL.host_fill(exe, tmp_path, scenes[name], origin, size, n, mask, winding, grid=arrays, page=page), want, f"sanitized walk {key}")
        FL.assert_fill_equal(FL.host_fill(exe, tmp_path, scenes[name], origin, size, n, 7, True), FL.fixture_case(fixture, key, 7, True), f"sanitized brute force {key}")
