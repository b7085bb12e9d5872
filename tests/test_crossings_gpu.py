"""Crossing queries on the GPU (hagrid_amd/csrc/crossings.hip): the device's records against the fixture tests/golden/crossings.npz on Cell and SmallCell
grids built on the device, with a traversal image present and ray binning on, with counters null; the batch totals against the host walk's; batch tails;
points with one and three directions under both vote rules, records null and stored; the lattice form; hostile rays against the brute force; a larger live
case against the host walk; the signed-distance snippet from torch tensors on torch's stream; a C++ program through the shim; the crossing-count picture;
every argument error; the kernel budget.  Every compared output comes from a poisoned, guarded buffer (tests/_poison.py).
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import ctypes as C
import sys

import numpy as np
import pytest

import _crossings as X
import _gpu_case as G
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(X.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("crossings_host_gpu")
    return X.build_host(d), d


@pytest.fixture(scope="module", params=X.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, the rays uploaded"""
    c = G.open_case(request.param, X.make_tris(request.param))
    c.fixture = fixture
    c.rays = fixture[c.name + "_rays"]
    c.want = fixture[c.name + "_records"]
    c.n = c.rays.shape[0]
    c.d_rays = c.mem.upload(c.rays)
    yield c
    c.mem.close()


def run_rays(c, grid, d_rays, n, counters=False):
    """records (n, 4) uint32 [, the four batch totals]"""
    mem = c.mem
    d_rec = P.alloc_out(mem, 16 * n)
    d_tot = 0
    if counters:
        d_tot = mem.alloc(32); mem.zero(d_tot, 32)
    c.api.count_crossings(grid, c.d_tris, d_rays, d_rec, n, d_tot)
    mem.synchronize()
    rec = P.fetch(mem, d_rec, np.uint32, 4 * n).reshape(n, 4)
    mem.free(d_rec)
    if not counters:
        return rec
    tot = mem.download(d_tot, np.int64, 4)
    mem.free(d_tot)
    return rec, tot


def run_points(c, grid, d_points, n, m, dirs=None, flags=0, records=True, counters=False, lattice=None):
    """(inside (n,), records (n * m, 4) uint32 or None[, totals])"""
    mem = c.mem
    d_in = P.alloc_out(mem, 4 * n)
    d_rec = P.alloc_out(mem, 16 * n * m) if records else 0
    d_tot = 0
    if counters:
        d_tot = mem.alloc(32); mem.zero(d_tot, 32)
    if lattice is None:
        c.api.points_inside(grid, c.d_tris, d_points, n, d_in, dirs, d_rec, d_tot, flags)
    else:
        c.api.inside_lattice(grid, c.d_tris, lattice[0], lattice[1], lattice[2], d_in, dirs, d_rec, d_tot, flags)
    mem.synchronize()
    out = [P.fetch(mem, d_in, np.int32, n), None]
    mem.free(d_in)
    if records:
        out[1] = P.fetch(mem, d_rec, np.uint32, 4 * n * m).reshape(n * m, 4)
        mem.free(d_rec)
    if counters:
        out.append(mem.download(d_tot, np.int64, 4))
        mem.free(d_tot)
    return out


@pytest.mark.parametrize("compress", [False, True])
def test_device_records_equal_the_fixture(case, compress):
    c = case
    c.mem.set_option("traverse.image", 0)
    try:
        X.assert_records_equal(run_rays(c, c.grids[compress], c.d_rays, c.n), c.want, f"{c.name} compress={compress}")
    finally:
        c.mem.set_option("traverse.image", 2)


@pytest.mark.parametrize("compress", [False, True])
def test_image_binning_and_null_counters(case, compress):
    """a traversal image and ray binning are ignored and survive; counters may be null (above) or given"""
    c = case; mem = c.mem
    grid = c.grids[compress]
    with G.image_present(c, grid):
        X.assert_records_equal(run_rays(c, grid, c.d_rays, c.n), c.want, f"{c.name} image present")
        mem.set_ray_binning(1)
        rec, tot = run_rays(c, grid, c.d_rays, c.n, counters=True)
        X.assert_records_equal(rec, c.want, f"{c.name} binning set, counters given")
        assert tot[0] == c.n


@pytest.mark.parametrize("compress", [False, True])
def test_batch_totals_equal_the_host_walk(case, host, compress):
    c = case
    exe, d = host
    grid = c.grids[compress]
    rec, tot = run_rays(c, grid, c.d_rays, c.n, counters=True)
    w = X.host_query(exe, d, c.tris, grid=grid.download(c.mem), page=8, rays=c.rays)
    X.assert_records_equal(rec, w["records"], f"{c.name} compress={compress} against the host walk over the device's grid")
    assert tot.tolist() == w["totals"].tolist() and tot[1] > 0 and tot[2] > 0 and tot[3] > 0
    # the totals are ADDED: a second launch doubles them
    d_rec = c.mem.alloc(16 * c.n)
    G.assert_totals_added(lambda d_tot: c.api.count_crossings(grid, c.d_tris, c.d_rays, d_rec, c.n, d_tot), c.mem, tot)
    c.mem.free(d_rec)


def test_batch_tails(case):
    """prefixes of 1, 63, 64, 65 and 129 rays: the tail of a wavefront writes nothing (the guard behind the records)"""
    c = case
    grid = c.grids[True]
    c.api.count_crossings(grid, c.d_tris, 0, 0, 0)                  # no rays: nothing is launched, null buffers are fine
    c.api.count_crossings(grid, 0, 0, 0, 0, 0)
    c.api.points_inside(grid, 0, 0, 0, 0)
    for n in (1, 63, 64, 65, 129):
        X.assert_records_equal(run_rays(c, grid, c.d_rays, n), c.want[:n], f"{c.name} n={n}")
    first = c.n - 65                                                 # the aimed rays with many crossings, at an offset into the buffer
    X.assert_records_equal(run_rays(c, grid, c.d_rays + 32 * first, 65), c.want[first:], f"{c.name} the last 65")


@pytest.fixture(scope="module")
def solids(fixture):
    c = G.upload_case(X.make_tris("solids"))
    c.fixture = fixture
    c.grids = {False: c.api.build_all(c.mem, c.d_tris, c.tris.shape[0]), True: c.api.build_all(c.mem, c.d_tris, c.tris.shape[0], compress=True)}
    c.pts = fixture["points"]
    c.d_pts = c.mem.upload(c.pts)
    yield c
    c.mem.close()


@pytest.mark.parametrize("compress", [False, True])
def test_points(solids, host, compress):
    """m = 1 and m = 3, both vote rules, records null and stored; the labels; the totals against the host walk"""
    c = solids; f = c.fixture
    exe, d = host
    grid = c.grids[compress]
    n = X.NUM_POINTS
    inside, rec, tot = run_points(c, grid, c.d_pts, n, 3, counters=True)
    X.assert_records_equal(rec, f["point_records"].reshape(-1, 4), "points m = 3")
    assert (inside == f["inside_m3"]).all() and (inside == f["labels"]).all()
    w = X.host_query(exe, d, c.tris, grid=grid.download(c.mem), page=8, points=c.pts)
    assert tot.tolist() == w["totals"].tolist()
    inside, rec = run_points(c, grid, c.d_pts, n, 3, records=False)
    assert rec is None and (inside == f["inside_m3"]).all()
    W = c.api.INSIDE_WINDING
    inside, rec = run_points(c, grid, c.d_pts, n, 3, flags=W)
    assert (inside == f["inside_m3_winding"]).all()
    X.assert_records_equal(rec, f["point_records"].reshape(-1, 4), "points m = 3, winding: the records do not depend on the vote rule")
    one = scene.CROSSING_DIRS[0:1]
    inside, rec = run_points(c, grid, c.d_pts, n, 1, dirs=one)
    assert (inside == f["inside_m1"]).all()
    X.assert_records_equal(rec, f["point_records"][:, 0, :], "points m = 1")
    inside, rec = run_points(c, grid, c.d_pts, n, 1, dirs=one, flags=W, records=False)
    assert (inside == f["inside_m1_winding"]).all()
    # the caller's three directions, tails, inactive points
    dirs = np.float32([[0, 0, 1], [0.6, 0, -0.8], [-1, 2, 0.5]])
    pts = c.pts[:131].copy()
    pts[5, 3] = -1.0; pts[6, 3] = np.nan; pts[7, 0] = np.nan; pts[8, 2] = np.inf; pts[9, 3] = 0.01
    d_p = c.mem.upload(pts)
    want = scene.points_inside(c.tris, pts, dirs=dirs)
    inside, rec = run_points(c, grid, d_p, 131, 3, dirs=dirs)
    assert (inside == want["inside"]).all() and (inside[5:9] == -1).all()
    X.assert_records_equal(rec, want["records"], "131 points, the caller's directions")
    c.mem.free(d_p)


def test_lattice(solids):
    c = solids; f = c.fixture
    lattice = (f["lattice_origin"], f["lattice_size"], f["lattice_n"])
    nv = int(np.prod(f["lattice_n"]))
    centres = scene.lattice_centres(*lattice)
    want = scene.points_inside(c.tris, centres)
    assert (want["inside"] == f["lattice_inside"]).all()
    for compress in (False, True):
        inside, rec = run_points(c, c.grids[compress], 0, nv, 3, lattice=lattice)
        assert (inside == f["lattice_inside"]).all()
        X.assert_records_equal(rec, want["records"], f"lattice compress={compress}")
    # a lattice that is no multiple of the wavefront, wider than the scene, one direction, the winding rule
    lo, hi = scene.tris_bbox(c.tris)
    n = (7, 5, 3)
    origin = (lo - np.float32(0.1) * (hi - lo)).astype(np.float32); size = (((hi - lo) * np.float32(1.2)) / np.float32(n)).astype(np.float32)
    want = scene.points_inside(c.tris, scene.lattice_centres(origin, size, n), dirs=scene.CROSSING_DIRS[1:2], winding=True)
    inside, rec = run_points(c, c.grids[True], 0, 105, 1, dirs=scene.CROSSING_DIRS[1:2], flags=c.api.INSIDE_WINDING, lattice=(origin, size, n))
    assert (inside == want["inside"]).all()
    X.assert_records_equal(rec, want["records"], "7 x 5 x 3 lattice")


@pytest.mark.parametrize("scene_name", ["soup", "mesh"])
def test_hostile_rays(host, scene_name):
    """the catalogue of tests/_hostile_rays.py at the grid's resolution against the header's brute force (families (i), (k), (l): X.assert_hostile_records) and,
    every family, against the host walk over the device's grid; inadmissible rays get the empty record"""
    import _hostile_rays as H
    from hagrid_amd import api
    exe, d = host
    tris = X.make_tris(scene_name)
    c = G.upload_case(tris); mem = c.mem
    # (the oracle's grid: the same resolution; Cell and SmallCell grids have the same voxel planes, so one catalogue and one brute force serve both)
    rays, family = H.catalogue(tris, X.oracle_grid(tris, False, True), mesh=scene_name == "mesh")
    want = X.host_query(exe, d, tris, rays=rays)["records"]
    d_rays = mem.upload(rays)
    for compress in (False, True):
        grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=compress)
        rec = run_rays(c, grid, d_rays, rays.shape[0])
        X.assert_hostile_records(rec, want, family, f"{scene_name} compress={compress}")
        walk = X.host_query(exe, d, tris, grid=grid.download(mem), page=8, rays=rays)["records"]
        X.assert_records_equal(rec, walk, "device = host walk over the same grid on EVERY family")
        refused = ~H._admissible(rays)
        assert refused.any() and (rec[refused] == X.empty_records(rays[refused])).all()
        grid.free()
    mem.free(d_rays)
    mem.close()


def test_larger_live_case(tmp_path):
    """100 000 triangles, 65 536 mixed rays (primary, incoherent, aimed through the scene, some with finite windows): the device's records against the host walk
    over the SAME grid arrays (downloaded), batch totals included, and against the numpy statement for the first 128 rays"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    lo, hi = scene.tris_bbox(tris)
    n = 65536
    rays = np.concatenate([scene.make_rays_primary(lo, hi, 128, 128), scene.make_rays_incoherent(lo, hi, 32768, 5), X.aimed_rays(tris, 16384, 6)]).astype(np.float32)
    rays[::7, 3] = np.float32(0.1); rays[::7, 7] = np.float32(0.9)
    rays = np.ascontiguousarray(rays[np.random.default_rng(5).permutation(n)])
    c = G.upload_case(tris); mem = c.mem
    d_rays = mem.upload(rays)
    exe = X.build_host(tmp_path)
    for compress in (False, True):
        grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=compress)
        rec, tot = run_rays(c, grid, d_rays, n, counters=True)
        w = X.host_query(exe, tmp_path, tris, grid=grid.download(mem), page=8, rays=rays)
        X.assert_records_equal(rec, w["records"], f"soup 100k compress={compress} against the host walk")
        assert tot.tolist() == w["totals"].tolist() and w["excess"] <= 0
        if not compress:
            X.assert_records_equal(rec[:128], scene.ray_crossings(tris, rays[:128]), "soup 100k against the statement")
            counts = rec[:, 0].view(np.int32)
            assert counts.max() > 16 and (counts == 0).any() and (counts > 8).sum() > 1000
        grid.free()
    mem.close()


def test_signed_distance_from_torch_tensors():
    """the snippet of INTEGRATION.md on torch's stream: sqrt(d2) * (1 - 2 * inside) from closest_points + points_inside, compared with numpy"""
    import torch
    from hagrid_amd import api
    tris, solids = scene.make_closed_solids(X.DETAIL)
    pts, labels = X.make_points(tris, solids)
    pts = pts[:1000]
    mem = api.MemManager(keep=True)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_tris = torch.from_numpy(tris).cuda()
            grid = api.build_all(mem, t_tris.data_ptr(), tris.shape[0])
            t_pts = torch.from_numpy(pts).cuda()                          # x, y, z, inf: the radius of closest_points and the reach of points_inside
            t_res = torch.full((pts.shape[0], 8), -7.0, dtype=torch.float32, device="cuda")
            t_in = torch.full((pts.shape[0],), -7, dtype=torch.int32, device="cuda")
            api.closest_points(grid, t_tris.data_ptr(), t_pts.data_ptr(), t_res.data_ptr(), pts.shape[0])
            api.points_inside(grid, t_tris.data_ptr(), t_pts.data_ptr(), pts.shape[0], t_in.data_ptr())
            sdf = torch.sqrt(t_res[:, 3]) * (1 - 2 * t_in).to(torch.float32)
            got = sdf.cpu().numpy(); inside = t_in.cpu().numpy()
            grid.free()
        stream.synchronize()
    finally:
        mem.use_stream(None)
    mem.close()
    assert (inside == labels[:1000]).all()
    d2 = scene.closest_points(tris, pts)["d2"]
    want = np.sqrt(d2).astype(np.float32) * (1 - 2 * scene.points_inside(tris, pts)["inside"]).astype(np.float32)
    # torch's sqrt and numpy's are each within an ulp of the root: two ulp between them at the most; the sign is exact
    assert (np.signbit(got) == np.signbit(want)).all() and np.allclose(got, want, rtol=2.0 ** -22, atol=0.0)
    assert (got < 0).sum() > 200 and (got > 0).sum() > 200


def test_cpp_program_through_the_shim(tmp_path):
    import _subproc
    r = _subproc.check([G.build_shim("crossings", tmp_path), "20000", "1000"], timeout=120)
    sys.stdout.write(r.stdout)
    assert " 0 mismatches vs host brute force" in r.stdout and " 0 mismatches in the point form" in r.stdout and " 0 mismatches in the lattice form" in r.stdout, r.stdout


def test_crossing_count_picture(case):
    """hagrid_shade_hits(GRAY) reads the records as they are: the picture is scene.shade_hits of the same array"""
    c = case; mem = c.mem
    d_rec = P.alloc_out(mem, 16 * c.n)
    c.api.count_crossings(c.grids[False], c.d_tris, c.d_rays, d_rec, c.n)
    for mode, clip in ((c.api.SHADE_GRAY, 0.0), (c.api.SHADE_HEAT, 0.0), (c.api.SHADE_DEPTH, 2.0)):
        d_px = P.alloc_out(mem, 4 * c.n)
        c.api.shade_hits(mem, d_rec, c.n, mode, clip, d_px)
        mem.synchronize()
        px = P.fetch(mem, d_px, np.uint8, 4 * c.n).reshape(c.n, 4)
        mem.free(d_px)
        assert (px == scene.shade_hits(c.want.view(scene.HIT_DTYPE).reshape(-1), mode, clip)).all()
    assert len(set(px[:, 0].tolist())) > 3
    mem.free(d_rec)


def test_errors_leave_the_context_working(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    n = 256
    d_rec = mem.alloc(16 * 3 * n + 64); d_in = mem.alloc(4 * n + 64); d_tot = mem.alloc(64)
    d_pts = mem.upload(np.zeros((n, 4), np.float32))
    EINVAL, ERANGE = G.EINVAL, G.ERANGE
    pod, vp = G.pod, G.vp

    def floats(dirs):
        return (C.c_float * len(dirs))(*dirs) if dirs is not None else None

    def rays(g, tris, r, rec, k, counters=0, flags=0):
        return L.hagrid_count_crossings(mem._ctx, pod(g), vp(tris), vp(r), vp(rec), k, vp(counters), flags)

    def points(g, tris, p, k, dirs, m, inside, rec=0, counters=0, flags=0):
        return L.hagrid_points_inside(mem._ctx, pod(g), vp(tris), vp(p), k, floats(dirs), m, vp(inside), vp(rec), vp(counters), flags)

    def lattice(g, origin, size, k, inside, dirs=None, m=0, rec=0, counters=0, flags=0, tris=None):
        return L.hagrid_inside_lattice(mem._ctx, pod(g), vp(c.d_tris if tris is None else tris), G.f3(origin), G.f3(size), G.i3(k), floats(dirs), m, vp(inside), vp(rec), vp(counters), flags)

    T, R = c.d_tris, c.d_rays
    assert rays(grid, T, R, d_rec, n, d_tot) == 0 and points(grid, T, d_pts, n, None, 0, d_in, d_rec, d_tot) == 0 and lattice(grid, (0, 0, 0), (1, 1, 1), (4, 4, 2), d_in, rec=d_rec) == 0
    # a null grid, null buffers, misaligned buffers
    assert rays(None, T, R, d_rec, n) == EINVAL and b"grid" in L.hagrid_last_error(mem._ctx)
    assert points(None, T, d_pts, n, None, 0, d_in) == EINVAL and lattice(None, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in) == EINVAL
    assert rays(grid, 0, R, d_rec, n) == EINVAL and rays(grid, T, 0, d_rec, n) == EINVAL and rays(grid, T, R, 0, n) == EINVAL
    assert points(grid, 0, d_pts, n, None, 0, d_in) == EINVAL and points(grid, T, 0, n, None, 0, d_in) == EINVAL and points(grid, T, d_pts, n, None, 0, 0) == EINVAL
    assert lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), 0) == EINVAL and lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in, tris=0) == EINVAL
    assert rays(grid, T + 4, R, d_rec, n) == EINVAL and rays(grid, T, R + 8, d_rec, n) == EINVAL and rays(grid, T, R, d_rec + 4, n) == EINVAL
    assert b"aligned" in L.hagrid_last_error(mem._ctx)
    assert rays(grid, T, R, d_rec, n, d_tot + 4) == EINVAL
    assert points(grid, T, d_pts + 8, n - 1, None, 0, d_in) == EINVAL and points(grid, T, d_pts, n, None, 0, d_in + 2) == EINVAL
    assert points(grid, T, d_pts, n, None, 0, d_in, d_rec + 8) == EINVAL and points(grid, T, d_pts, n, None, 0, d_in, d_rec, d_tot + 4) == EINVAL
    assert lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in + 2) == EINVAL and lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in, rec=d_rec + 4) == EINVAL
    # flags
    for flags in (1, 2, 1 << 31):
        assert rays(grid, T, R, d_rec, n, flags=flags) == EINVAL and b"flag" in L.hagrid_last_error(mem._ctx)
    for flags in (2, 3, 4, 1 << 31):
        assert points(grid, T, d_pts, n, None, 0, d_in, flags=flags) == EINVAL and lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in, flags=flags) == EINVAL
    # counts
    assert rays(grid, T, R, d_rec, -1) == EINVAL and points(grid, T, d_pts, -1, None, 0, d_in) == EINVAL
    assert L.hagrid_count_crossings(None, pod(grid), vp(T), vp(R), vp(d_rec), n, None, 0) == EINVAL
    # directions
    one = (0.0, 0.0, 1.0)
    for m in (-1, 2, 4):
        assert points(grid, T, d_pts, n, one * 4, m, d_in) == EINVAL and b"num_dirs" in L.hagrid_last_error(mem._ctx)
        assert lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in, one * 4, m) == EINVAL
    assert points(grid, T, d_pts, n, one, 0, d_in) == EINVAL and points(grid, T, d_pts, n, None, 1, d_in) == EINVAL and points(grid, T, d_pts, n, None, 3, d_in) == EINVAL
    for bad in ((0.0, 0.0, 0.0), (float("nan"), 0.0, 1.0), (0.0, float("inf"), 1.0), (1e-42, 0.0, -0.0)):
        assert points(grid, T, d_pts, n, bad, 1, d_in) == EINVAL and b"direction" in L.hagrid_last_error(mem._ctx)
        assert points(grid, T, d_pts, n, one + one + bad, 3, d_in) == EINVAL and lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in, bad, 1) == EINVAL
    assert points(grid, T, d_pts, n, one, 1, d_in) == 0
    # num_points * m beyond 2^31 - 1 (refused before anything is read)
    assert points(grid, T, d_pts, 1 << 30, None, 0, d_in) == ERANGE and points(grid, T, d_pts, (1 << 31) - 1, one, 1, 0) == EINVAL
    assert lattice(grid, (0, 0, 0), (1, 1, 1), (1 << 10, 1 << 10, 1 << 10), d_in) == ERANGE
    # the lattice errors of hagrid_overlap_lattice
    G.assert_lattice_refused(lambda origin, size, k: lattice(grid, origin, size, k, d_in))
    with pytest.raises(api.HagridError, match="aligned"):
        api.count_crossings(grid, T, R + 4, d_rec, 8)
    with pytest.raises(api.HagridError, match="voxel"):
        api.inside_lattice(grid, T, (0, 0, 0), (1, 1, 1), (0, 1, 1), d_in)
    # "traverse.id_is_steps" = 1
    mem.set_option("traverse.id_is_steps", 1)
    try:
        with pytest.raises(api.HagridError, match="id_is_steps"):
            api.count_crossings(grid, T, R, d_rec, n)
        assert points(grid, T, d_pts, n, None, 0, d_in) == EINVAL and lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in) == EINVAL
    finally:
        mem.set_option("traverse.id_is_steps", 0)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.count_crossings(g2, T, R, d_rec, n)
            with pytest.raises(api.HagridError, match="released"):
                api.points_inside(g2, T, d_pts, n, d_in)
            with pytest.raises(api.HagridError, match="released"):
                api.inside_lattice(g2, T, (0, 0, 0), (1, 1, 1), (2, 2, 2), d_in)
            assert rays(g2, T, R, d_rec, 0) == EINVAL
    mem.free(d_rec); mem.free(d_in); mem.free(d_tot); mem.free(d_pts)
    api.setup_traversal(grid)
    X.assert_records_equal(run_rays(c, grid, c.d_rays, c.n), c.want, f"{c.name} after the refused calls")


def test_kernel_budget():
    G.kernel_budget(G.kernel_listing(), one_each=("crossings_kernel", "bw_stream_kernel"), absent=("bw_copy_kernel", "bw_triad_kernel"))   # crossing queries are ONE kernel
