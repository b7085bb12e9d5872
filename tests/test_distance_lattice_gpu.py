"""The distance lattice by scatter on the GPU (hagrid_distance_lattice, hagrid_amd/csrc/distance.hip): every case of the fixture tests/golden/distance_lattice.npz on
Cell and SmallCell grids built on the device -- ids, d2 and records bit for bit, the records also against hagrid_closest_points on the device; a workspace
pre-filled with zeros (the smallest key: a missing initialisation shows); task shapes (one triangle alone, every triangle's box the whole lattice, 20 000 triangles
on 1 680 voxels); two launches with identical bits; the counters against numpy; each output null alone; every argument error; a C++ program through the shim;
api.signed_distance_lattice against the analytic solids; the kernel budget.  Every compared output comes from a poisoned, guarded buffer (tests/_poison.py).
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import ctypes as C
import sys

import numpy as np
import pytest

import _distance as D
import _fill_lattice as FL
import _gpu_case as G
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

SCENES = ("boxes", "soup", "mesh", "solids")


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(D.FIXTURE))


@pytest.fixture(scope="module", params=SCENES)
def case(request):
    """one scene of the fixture: Cell and SmallCell grids built on the device"""
    c = G.open_case(request.param, D.tris_of(request.param))
    c.lattices = [lat for lat in FL.lattices(c.name, c.tris) if lat[0] in D.KEYS]
    yield c
    c.mem.close()


def small_case(tris):
    c = G.upload_case(np.ascontiguousarray(tris, dtype=np.float32))
    c.grid = c.api.build_all(c.mem, c.d_tris, c.tris.shape[0])
    return c


def run_distance(c, grid, origin, size, n, band, ids=True, d2=True, records=True, counters=True):
    """"ids" int32, "d2" float32, "records" CLOSEST_DTYPE per voxel (None where not asked for), "totals" int64[4] or None.  The workspace is pre-filled with zeros,
    with a guard behind it; the outputs are poisoned and guarded."""
    mem = c.mem
    voxels = int(np.prod([int(v) for v in n]))
    d_ws = P.alloc_out(mem, 8 * voxels); mem.zero(d_ws, 8 * voxels)
    d_ids = P.alloc_out(mem, 4 * voxels) if ids else 0
    d_d2 = P.alloc_out(mem, 4 * voxels) if d2 else 0
    d_rec = P.alloc_out(mem, 32 * voxels) if records else 0
    d_tot = 0
    if counters:
        d_tot = mem.alloc(32); mem.zero(d_tot, 32)
    c.api.distance_lattice(grid, c.d_tris, origin, size, n, band, d_ws, ids=d_ids, d2=d_d2, records=d_rec, counters=d_tot)
    mem.synchronize()
    P.fetch(mem, d_ws, np.uint64, voxels)               # (the guard behind the workspace; its content is unspecified)
    mem.free(d_ws)
    out = {"ids": None, "d2": None, "records": None, "totals": None}
    if ids:
        out["ids"] = P.fetch(mem, d_ids, np.int32, voxels).copy(); mem.free(d_ids)
    if d2:
        out["d2"] = P.fetch(mem, d_d2, np.float32, voxels).copy(); mem.free(d_d2)
    if records:
        out["records"] = P.fetch(mem, d_rec, scene.CLOSEST_DTYPE, voxels).copy(); mem.free(d_rec)
    if counters:
        out["totals"] = mem.download(d_tot, np.int64, 4); mem.free(d_tot)
    return out


def assert_equal(got, want, what):
    """ids, d2 (bits) and the 32-byte records against CLOSEST_DTYPE records"""
    if got["ids"] is not None:
        bad = got["ids"] != want["id"]
        assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} ids differ, first at {np.flatnonzero(bad)[:5]}: got {got['ids'][bad][:5]}, want {want['id'][bad][:5]}"
    if got["d2"] is not None:
        bad = got["d2"].view(np.uint32) != want["d2"].view(np.uint32)
        assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} d2 differ, first at {np.flatnonzero(bad)[:5]}: got {got['d2'][bad][:5]}, want {want['d2'][bad][:5]}"
    if got["records"] is not None:
        D.assert_records_equal(got["records"], want, what)


@pytest.mark.parametrize("compress", [False, True])
def test_device_equals_the_fixture(case, fixture, compress):
    """every lattice of the scene, both bands: ids, d2 and records are the fixture's; pairs within the band and voxels found are numpy's"""
    c = case
    for key, origin, size, n in c.lattices:
        for b, f in enumerate(D.BAND_FACTORS):
            band = D.band_of(size, f)
            want = D.fixture_records(fixture, key, b)
            got = run_distance(c, c.grids[compress], origin, size, n, band)
            assert_equal(got, want, f"{key} band {f} compress={compress}")
            t = got["totals"]
            assert t[2] == fixture[key + "_pairs"][b] and t[3] == (want["id"] >= 0).sum() and 0 < t[0] <= c.tris.shape[0] and t[1] >= t[0], t


def test_records_are_those_of_closest_points_on_the_device(case):
    c = case; mem = c.mem
    key, origin, size, n = c.lattices[-1]
    band = D.band_of(size, D.BAND_FACTORS[0])
    pts = scene.lattice_centres(origin, size, n); pts["r"] = band
    d_pts = mem.upload(pts)
    d_res = P.alloc_out(mem, 32 * pts.size)
    c.api.closest_points(c.grids[False], c.d_tris, d_pts, d_res, pts.size)
    mem.synchronize()
    want = P.fetch(mem, d_res, scene.CLOSEST_DTYPE, pts.size).copy()
    mem.free(d_res); mem.free(d_pts)
    got = run_distance(c, c.grids[False], origin, size, n, band)
    assert_equal(got, want, f"{key}: against hagrid_closest_points")
    assert (want["id"] >= 0).any()


def test_two_launches_give_identical_bits(case):
    c = case
    key, origin, size, n = c.lattices[0]
    band = D.band_of(size, D.BAND_FACTORS[1])
    a = run_distance(c, c.grids[True], origin, size, n, band)
    b = run_distance(c, c.grids[True], origin, size, n, band)
    assert (a["ids"] == b["ids"]).all() and (a["d2"].view(np.uint32) == b["d2"].view(np.uint32)).all()
    assert (a["records"].view(np.uint32) == b["records"].view(np.uint32)).all() and (a["totals"] == b["totals"]).all()


def test_each_output_may_be_null_alone_and_counters_are_added(case, fixture):
    c = case; mem = c.mem
    key, origin, size, n = c.lattices[0]
    band = D.band_of(size, D.BAND_FACTORS[0])
    want = D.fixture_records(fixture, key, 0)
    for ids, d2, records in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True), (True, False, True)):
        got = run_distance(c, c.grids[False], origin, size, n, band, ids=ids, d2=d2, records=records, counters=records)
        assert (got["ids"] is not None) == ids and (got["d2"] is not None) == d2 and (got["records"] is not None) == records
        assert_equal(got, want, f"{key}: ids={ids} d2={d2} records={records}")
    full = run_distance(c, c.grids[False], origin, size, n, band)["totals"]
    voxels = int(np.prod(n))
    d_ws = mem.alloc(8 * voxels); d_ids = mem.alloc(4 * voxels)
    G.assert_totals_added(lambda d_tot: c.api.distance_lattice(c.grids[False], c.d_tris, origin, size, n, band, d_ws, ids=d_ids, counters=d_tot), mem, full)
    mem.free(d_ws); mem.free(d_ids)


def test_with_and_without_the_traversal_image(case, fixture):
    """the triangle count comes from the context's traversal image when it belongs to the grid, else from a pass over the references: the same answers; the query
    leaves the image alone"""
    c = case; mem = c.mem
    key, origin, size, n = c.lattices[0]
    band = D.band_of(size, D.BAND_FACTORS[0])
    want = D.fixture_records(fixture, key, 0)
    mem.set_option("traverse.image", 2)
    c.api.setup_traversal(c.grids[False])
    with_image = mem.image_bytes(c.grids[False]) > 0
    assert_equal(run_distance(c, c.grids[False], origin, size, n, band), want, f"{key}: image of this grid")
    assert_equal(run_distance(c, c.grids[True], origin, size, n, band), want, f"{key}: image of another grid")
    assert (mem.image_bytes(c.grids[False]) > 0) == with_image, "the query dropped the traversal image"


def test_one_triangle_alone():
    """fewer tasks than wavefronts: one task (a narrow band) and a few (a band that covers the lattice)"""
    v = np.float32([[0.0, 0.0, 0.0], [1.0, 0.2, 0.1], [0.1, 1.0, 0.3]])
    c = small_case(scene.tris_from_vertices(v[0:1], v[1:2], v[2:3]))
    origin, size, n = np.float32([-0.35, -0.3, -0.45]), np.float32([0.07, 0.09, 0.11]), (23, 17, 11)
    for band in (0.1, 5.0):
        got = run_distance(c, c.grid, origin, size, n, band)
        want = scene.distance_lattice(c.tris, origin, size, n, band)
        assert_equal(got, want, f"one triangle, band {band}")
        t = got["totals"].tolist()
        assert [t[0], t[2], t[3]] == [1, int((want["id"] >= 0).sum()), int((want["id"] >= 0).sum())]
        assert t[1] == 3 if band == 5.0 else 1 <= t[1] <= 3, t          # 23 * 17 * 11 = 4 301 voxels: three tasks when the box is the whole lattice
        assert 0 < (want["id"] >= 0).sum() and ((want["id"] >= 0).all() == (band == 5.0))
    c.grid.free(); c.mem.close()


def test_several_tasks_per_triangle(case):
    """boxes on boxes_c: with band 0.75 every triangle's box spans the lattice in y and z and most of it in x (two or three tasks each); with band 2.5 it is the
    whole lattice of 7 168 voxels, four tasks each, and every voxel is offered every triangle"""
    c = case
    if c.name != "boxes":
        return
    tris, origin, size, n = D.case("boxes_c")
    for band in (0.75, 2.5):
        got = run_distance(c, c.grids[False], origin, size, n, band)
        want = scene.distance_lattice(tris, origin, size, n, band)
        assert_equal(got, want, f"boxes_c band {band}")
        t = got["totals"]
        assert t[0] == 24 and t[2] == D.pairs_within(tris, origin, size, n, band) and t[3] == (want["id"] >= 0).sum()
        assert t[1] == 24 * 4 if band == 2.5 else 24 * 2 <= t[1] < 24 * 4, t
    # band 0: exactly the centres ON the surface, every tie to the smallest id (the fixture of the CPU test states which)
    got = run_distance(c, c.grids[True], origin, size, n, 0.0)
    want = scene.distance_lattice(tris, origin, size, n, 0.0)
    assert_equal(got, want, "boxes_c band 0")
    _, on = FL.boxes_truth(FL.centres(origin, size, n))
    assert ((got["ids"] >= 0) == on).all()


def test_other_lattices(case):
    """one voxel, a flat lattice, a lattice outside the scene, centres that overflow, voxels an ulp wide"""
    c = case
    if c.name != "boxes":
        return
    for key in ("boxes_one", "boxes_flat"):
        tris, origin, size, n = D.case(key)
        for f in (0.5, 1.5):
            band = D.band_of(size, f)
            assert_equal(run_distance(c, c.grids[False], origin, size, n, band), scene.distance_lattice(tris, origin, size, n, band), f"{key} band {f}")
    origin, size, n = np.float32([10.0, -7.0, 3.0]), np.float32([0.25, 0.5, 0.125]), (9, 5, 7)
    got = run_distance(c, c.grids[False], origin, size, n, 0.7)
    assert_equal(got, scene.distance_lattice(c.tris, origin, size, n, 0.7), "outside the scene")
    assert (got["ids"] == -1).all() and (got["d2"] == np.float32(0.7) * np.float32(0.7)).all() and got["totals"].tolist() == [0, 0, 0, 0]
    origin, size, n = np.float32([3e38, 0.1, 0.1]), np.float32([3e38, 0.2, 0.2]), (3, 2, 2)
    with np.errstate(all="ignore"):
        want = scene.distance_lattice(c.tris, origin, size, n, 0.5)
    got = run_distance(c, c.grids[True], origin, size, n, 0.5)
    assert_equal(got, want, "overflowed centres")
    assert (got["ids"] == -1).all()
    origin, size, n, band = np.float32([0.999995, 0.3, 0.3]), np.float32([3e-8, 0.2, 0.2]), (1000, 3, 3), 2e-7
    want = scene.distance_lattice(c.tris, origin, size, n, band)
    assert_equal(run_distance(c, c.grids[False], origin, size, n, band), want, "voxels an ulp wide")
    assert 0.007 <= (want["id"] >= 0).mean() <= 0.03


def test_triangles_without_a_surface_never_win():
    base, origin, size, n = D.case("boxes_a")
    centres = FL.centres(origin, size, n)
    ghosts = base.copy(); ghosts[:, 3] = 0; ghosts[:, 7] = 0; ghosts[:, 11] = 0
    points = np.zeros((8, 12), np.float32); points[:, 0:3] = centres[::113][:8]
    c = small_case(np.concatenate([ghosts[:5], points, base, ghosts[5:]]))
    band = D.band_of(size, 1.5)
    got = run_distance(c, c.grid, origin, size, n, band)
    assert_equal(got, scene.distance_lattice(c.tris, origin, size, n, band), "zero-normal triangles mixed in")
    found = got["ids"] >= 0
    assert found.any() and (got["ids"][found] >= 13).all() and (got["ids"][found] < 13 + base.shape[0]).all() and got["totals"][0] == base.shape[0]
    c.grid.free(); c.mem.close()


def test_signed_distance_lattice_on_the_solids(fixture):
    """api.signed_distance_lattice on torch's stream (lattice solids_a, band = 3 voxels): the sign is the analytic solids' for every voxel farther than NEAR from the
    analytic surface; where a triangle was found | |sdf| - analytic distance | <= NEAR; sdf = +-sqrt(d2) of numpy within 1 ulp"""
    import torch
    from hagrid_amd import api
    tris, origin, size, n = D.case("solids_a")
    nx, ny, nz = (int(v) for v in n)
    band = D.band_of(size, 3.0)
    mem = api.MemManager(keep=True)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_tris = torch.from_numpy(tris).cuda()
            grid = api.build_all(mem, t_tris.data_ptr(), tris.shape[0])
            out = api.signed_distance_lattice(grid, t_tris, origin, size, n, band)
            assert set(out) == {"sdf", "d2", "ids", "inside"}
            for k, dt in (("sdf", torch.float32), ("d2", torch.float32), ("ids", torch.int32), ("inside", torch.int32)):
                assert out[k].dtype == dt and tuple(out[k].shape) == (nz, ny, nx)
            got = {k: v.cpu().numpy().reshape(-1) for k, v in out.items()}
            grid.free()
        stream.synchronize()
    finally:
        mem.use_stream(None)
    mem.close()
    want = D.fixture_records(fixture, "solids_a", 1)
    assert (got["ids"] == want["id"]).all() and (got["d2"].view(np.uint32) == want["d2"].view(np.uint32)).all()
    assert (got["inside"] == fixture_fill()["solids_a_inside"][1, 6]).all()
    truth, dist = FL.solids_truth(FL.centres(origin, size, n))
    far = dist > FL.NEAR
    assert far.sum() > 0.5 * far.size and ((got["sdf"] < 0) == (truth == 1))[far].all()
    found = got["ids"] >= 0
    assert 0.5 < found.mean() < 0.6
    assert (np.abs(np.abs(got["sdf"][found].astype(np.float64)) - dist[found]) <= FL.NEAR).all()
    ref = np.sqrt(want["d2"]).astype(np.float32) * np.where(got["inside"] == 1, np.float32(-1.0), np.float32(1.0))
    assert (np.abs(got["sdf"] - ref) <= np.spacing(np.abs(ref))).all()
    assert (np.abs(got["sdf"][~found]) == np.sqrt(band * band)).all(), "no triangle within the band: +-band"


def fixture_fill():
    return np.load(FL.FIXTURE)


def test_cpp_program_through_the_shim(tmp_path):
    import _subproc
    r = _subproc.check([G.build_shim("distance", tmp_path), "40"], timeout=120)
    sys.stdout.write(r.stdout)
    assert " 0 ids or d2 differ, 0 records differ" in r.stdout, r.stdout


def test_errors_leave_the_context_working(case, fixture):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    key, origin, size, n = c.lattices[0]
    voxels = int(np.prod(n))
    d_ws = mem.alloc(8 * voxels + 64); d_ids = mem.alloc(4 * voxels + 64); d_d2 = mem.alloc(4 * voxels + 64); d_rec = mem.alloc(32 * voxels + 64); d_tot = mem.alloc(64)
    mem.zero(d_tot, 64)
    band = float(D.band_of(size, 1.5))
    EINVAL = G.EINVAL
    vp = G.vp

    def call(g=grid, tris=c.d_tris, o=origin, s=size, k=n, r=band, work=d_ws, ids=d_ids, d2=d_d2, records=d_rec, counters=d_tot, flags=0, ctx=mem._ctx):
        return L.hagrid_distance_lattice(ctx, G.pod(g), vp(tris), G.f3(o), G.f3(s), G.i3(k), C.c_float(r), vp(work), vp(ids), vp(d2), vp(records), vp(counters), flags)

    assert call() == 0 and call(records=0, counters=0) == 0 and call(ids=0, d2=0) == 0 and call(r=0.0) == 0
    # a null context, a null grid, null buffers
    assert call(ctx=None) == EINVAL
    assert call(g=None) == EINVAL and b"grid" in L.hagrid_last_error(mem._ctx)
    assert call(tris=0) == EINVAL and b"null" in L.hagrid_last_error(mem._ctx)
    # the band
    for r in (-1.0, -1e-30, np.nan, np.inf, -np.inf):
        assert call(r=r) == EINVAL and b"band" in L.hagrid_last_error(mem._ctx)
    # the workspace, and an output
    assert call(work=0) == EINVAL and call(work=d_ws + 4) == EINVAL and b"workspace" in L.hagrid_last_error(mem._ctx)
    assert call(ids=0, d2=0, records=0) == EINVAL and b"at least one" in L.hagrid_last_error(mem._ctx)
    # misaligned buffers
    assert call(ids=d_ids + 2) == EINVAL and call(d2=d_d2 + 1) == EINVAL and call(counters=d_tot + 4) == EINVAL and b"aligned" in L.hagrid_last_error(mem._ctx)
    assert call(tris=c.d_tris + 4) == EINVAL and call(records=d_rec + 8) == EINVAL and b"aligned" in L.hagrid_last_error(mem._ctx)
    assert call(ids=d_ids + 4, d2=d_d2 + 12, work=d_ws + 8, records=d_rec + 16) == 0
    # the lattice, null arrays among its cases
    G.assert_lattice_refused(lambda o, s, k: call(o=o, s=s, k=k))
    assert call(k=(4, 4, 0)) == EINVAL and b"voxel" in L.hagrid_last_error(mem._ctx)
    # any flag
    for flags in (1, 2, 1 << 31):
        assert call(flags=flags) == EINVAL and b"flag" in L.hagrid_last_error(mem._ctx)
    with pytest.raises(api.HagridError, match="workspace"):
        api.distance_lattice(grid, c.d_tris, origin, size, n, band, 0, ids=d_ids)
    with pytest.raises(api.HagridError, match="band"):
        api.distance_lattice(grid, c.d_tris, origin, size, n, -0.5, d_ws, ids=d_ids)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.distance_lattice(g2, c.d_tris, origin, size, n, band, d_ws, ids=d_ids)
    mem.free(d_ws); mem.free(d_ids); mem.free(d_d2); mem.free(d_rec); mem.free(d_tot)
    got = run_distance(c, grid, origin, size, n, band)
    assert_equal(got, D.fixture_records(fixture, key, 0), f"{key} after the refused calls")


def test_kernel_budget():
    """one kernel with three modes; the slot came from the two ray generators of frame.hip, now one kernel"""
    from hagrid_amd import lib
    assert "hagrid_distance_lattice" in lib.SIGNATURES
    G.kernel_budget(G.kernel_listing(), one_each=("distance_kernel",))         # the distance lattice is ONE kernel
