"""Multi-hit traversal on the GPU (hagrid_amd/csrc/trav_multi.hip): the device's lists against the fixture tests/golden/multi_hit.npz
(ids equal, t bit-equal, no ray excepted) for every k bucket, both cell formats, with and without a traversal image, with ray binning
switched on; barycentrics against the oracle; a larger live case against the host walk and the per-triangle brute force; edges and
error cases; no interference with the nearest-hit path; hagrid_shade_layers against scene.shade_layers.
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import ctypes as C

import numpy as np
import pytest

import _gpu_case as G
import _multi_hit as M
from _poison import alloc_out, assert_all_written, fetch
from hagrid_amd import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(M.FIXTURE)


@pytest.fixture(scope="module", params=M.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, the rays uploaded"""
    c = G.open_case(request.param, M.make_tris(request.param))
    c.rays, c.ids, c.t = fixture[c.name + "_rays"], fixture[c.name + "_ids"], fixture[c.name + "_t"]
    c.n = c.rays.shape[0]
    c.d_rays = c.mem.upload(c.rays)
    yield c
    c.mem.close()


def run_multi(c, grid, d_rays, n, k, flags=0):
    """the lists of n rays as an (n, k) HIT_DTYPE array out of a poisoned buffer whose guard must stay untouched"""
    mem = c.mem
    d_hits = alloc_out(mem, 16 * n * k)
    c.api.traverse_grid_multi(grid, c.d_tris, d_rays, d_hits, n, k, flags)
    mem.synchronize()
    got = fetch(mem, d_hits, c.api.HIT_DTYPE, n * k).copy()
    mem.free(d_hits)
    return got.reshape(n, k)


def assert_lists(got, ids, t, what):
    k = got.shape[1]
    bad = (got["id"] != ids[:, :k]).any(axis=1) | (M.bits(got["t"]) != M.bits(t[:, :k])).any(axis=1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} rays differ, first at {np.flatnonzero(bad)[:5]}"


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("compress", [False, True])
def test_device_lists_equal_the_fixture(case, compress, k):
    c = case
    c.mem.set_option("traverse.image", 0)
    got = run_multi(c, c.grids[compress], c.d_rays, c.n, k)
    assert_lists(got, c.ids, c.t, f"{c.name} compress={compress} k={k}")
    assert (got["u"] == 0).all() and (got["v"] == 0).all()
    c.mem.set_option("traverse.image", 2)


@pytest.mark.parametrize("compress", [False, True])
def test_image_and_ray_binning_are_ignored(case, compress):
    c = case; mem = c.mem
    grid = c.grids[compress]
    with G.image_present(c, grid):
        for k in (1, 4, 8):
            assert_lists(run_multi(c, grid, c.d_rays, c.n, k), c.ids, c.t, f"{c.name} image present k={k}")
        mem.set_ray_binning(1)
        for k in (2, 8):
            assert_lists(run_multi(c, grid, c.d_rays, c.n, k), c.ids, c.t, f"{c.name} binning set k={k}")
    G.drop_image(c, grid)
    assert_lists(run_multi(c, grid, c.d_rays, c.n, 8), c.ids, c.t, f"{c.name} traverse.image=0")
    mem.set_option("traverse.image", 2)


@pytest.mark.parametrize("k", [2, 8])
def test_barycentrics(case, k):
    """with HAGRID_TRAVERSE_UVS u and v of every reported (ray, id) are the oracle's for that pair, bit for bit; ids and t do not move"""
    from oracle import oracle as O
    c = case
    got = run_multi(c, c.grids[False], c.d_rays, c.n, k, flags=c.api.UVS)
    assert_lists(got, c.ids, c.t, f"{c.name} uvs k={k}")
    L = O.lib()
    rows, cols = np.nonzero(got["id"] >= 0)
    assert rows.size > 1000
    tris = np.ascontiguousarray(c.tris, dtype=np.float32); rays = np.ascontiguousarray(c.rays, dtype=np.float32)
    h = np.zeros(1, dtype=O.HIT_DTYPE)
    want_u = np.empty(rows.size, dtype=np.float32); want_v = np.empty(rows.size, dtype=np.float32)
    for n, (i, j) in enumerate(zip(rows, cols)):
        tid = int(got["id"][i, j])
        assert L.orc_intersect_prim_ray_uv(tris[tid].ctypes.data_as(C.c_void_p), rays[i].ctypes.data_as(C.c_void_p), tid, h.ctypes.data_as(C.c_void_p)) == 1
        assert h["t"][0].view(np.uint32) == got["t"][i, j].view(np.uint32)
        want_u[n] = h["u"][0]; want_v[n] = h["v"][0]
    assert (M.bits(got["u"][rows, cols]) == M.bits(want_u)).all() and (M.bits(got["v"][rows, cols]) == M.bits(want_v)).all()
    assert (want_u != 0).any() and (want_v != 0).any()
    unused = got["id"] < 0
    assert (got["u"][unused] == 0).all() and (got["v"][unused] == 0).all()


def test_prefix_property(case):
    c = case
    full = run_multi(c, c.grids[True], c.d_rays, c.n, 8)
    for k in (1, 3, 6, 7):
        got = run_multi(c, c.grids[True], c.d_rays, c.n, k)
        assert (got.view(np.uint32) == np.ascontiguousarray(full[:, :k]).view(np.uint32)).all()


def test_edges(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    # no rays: nothing is launched, null buffers are fine
    api.traverse_grid_multi(grid, c.d_tris, 0, 0, 0, 4)
    # a batch that is not a multiple of 64, at an offset into the ray buffer
    for n, first in ((1, 0), (63, 5), (1000, 64), (4095, 1)):
        got = run_multi(c, grid, c.d_rays + 32 * first, n, 5)
        assert_lists(got, c.ids[first:first + n], c.t[first:first + n], f"{c.name} n={n} first={first}")
    # inactive rays (tmax -1) among live ones: k empty slots with t = -1
    rays = c.rays[:640].copy()
    rays[::3] = scene.make_rays_inactive(rays[::3].shape[0])
    d = mem.upload(rays)
    got = run_multi(c, c.grids[True], d, rays.shape[0], 8)
    mem.free(d)
    assert (got["id"][::3] == -1).all() and (got["t"][::3] == np.float32(-1.0)).all() and (got["u"][::3] == 0).all()
    live = np.ones(rays.shape[0], dtype=bool); live[::3] = False
    assert_lists(got[live], c.ids[:640][live], c.t[:640][live], f"{c.name} live rays next to inactive ones")


def test_errors_leave_the_context_working(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    d_hits = mem.alloc(16 * 8 * c.n)
    for k in (0, -1, 9, 1 << 20):
        with pytest.raises(api.HagridError, match="HAGRID_MAX_HITS"):
            api.traverse_grid_multi(grid, c.d_tris, c.d_rays, d_hits, c.n, k)
    for flags in (api.ANY_HIT, api.ANY_HIT | api.UVS, 4, 8):
        with pytest.raises(api.HagridError, match="flag"):
            api.traverse_grid_multi(grid, c.d_tris, c.d_rays, d_hits, c.n, 4, flags)
    with pytest.raises(api.HagridError, match=r"failed \(-4\)"):                         # HAGRID_ERANGE: the range check comes before any launch
        api.traverse_grid_multi(grid, c.d_tris, c.d_rays, d_hits, (1 << 31) - 1, 2)
    mem.set_option("traverse.id_is_steps", 1)
    try:
        with pytest.raises(api.HagridError, match="id_is_steps"):
            api.traverse_grid_multi(grid, c.d_tris, c.d_rays, d_hits, c.n, 4)
    finally:
        mem.set_option("traverse.id_is_steps", 0)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.traverse_grid_multi(g2, c.d_tris, c.d_rays, d_hits, c.n, 4)
            api.traverse_grid(g2, c.d_tris, c.d_rays, d_hits, c.n)                     # ... and still serves the nearest hit
            mem.synchronize()
    mem.free(d_hits)
    assert_lists(run_multi(c, grid, c.d_rays, c.n, 8), c.ids, c.t, f"{c.name} after the refused calls")


def test_no_interference_with_the_nearest_hit_path(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    mem.set_option("traverse.image", 2)
    api.setup_traversal(grid)
    with G.nearest_hit_unmoved(c, grid, c.d_rays, c.n) as nearest:
        got = run_multi(c, grid, c.d_rays, c.n, 8)
    assert_lists(got, c.ids, c.t, c.name)
    # k = 1 is not promised to equal the nearest hit (a tie in t, the scaled tmax comparison), but a ray has a nearest hit exactly when its list
    # is not empty: the first triangle the nearest-hit walk accepts was tested against the ray's own window
    assert ((nearest.before["id"] >= 0) == (got["id"][:, 0] >= 0)).all()


@pytest.mark.parametrize("k,opacity", [(1, 1.0), (4, 0.5), (8, 0.3), (8, 1.0)])
def test_shade_layers_on_device_lists(case, k, opacity):
    c = case; api, mem = c.api, c.mem
    clip = float(c.rays[1, 7])
    d_hits = alloc_out(mem, 16 * c.n * k)
    d_px = mem.alloc(4 * c.n + 16)
    mem.one(d_px, 4 * c.n + 16)
    api.traverse_grid_multi(c.grids[True], c.d_tris, c.d_rays, d_hits, c.n, k)
    api.shade_layers(mem, d_hits, c.n, k, clip, opacity, d_px)
    mem.synchronize()
    px = mem.download(d_px, np.uint8, 4 * c.n + 16)
    lists = fetch(mem, d_hits, api.HIT_DTYPE, c.n * k).reshape(c.n, k)
    assert_all_written(lists.reshape(-1))
    assert_lists(lists, c.ids, c.t, f"{c.name} k={k} in front of the shader")
    assert (px[4 * c.n:] == 255).all(), "written beyond the pixels"
    want = scene.shade_layers(lists, k, clip, opacity)
    assert (px[:4 * c.n].reshape(c.n, 4) == want).all()
    assert len(np.unique(want[:, 0])) > 20
    for bad in ({"clip": 0.0}, {"clip": -1.0}, {"opacity": 0.0}, {"opacity": 1.5}, {"opacity": float("nan")}, {"k": 0}, {"k": 9}):
        a = {"clip": clip, "opacity": opacity, "k": k}; a.update(bad)
        with pytest.raises(api.HagridError):
            api.shade_layers(mem, d_hits, c.n, a["k"], a["clip"], a["opacity"], d_px)
    mem.free(d_hits); mem.free(d_px)


def test_larger_live_case(tmp_path):
    """100 000 triangles, 65 536 rays (half primary, half incoherent, every fifth with a finite window), k = 8: the device's lists against
    the host walk over the SAME grid arrays (downloaded), and against the per-triangle brute force for the first 1024 rays"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    rays = M.mixed_rays(tris, 256, 128, 32768)
    rays = np.ascontiguousarray(rays[np.random.default_rng(5).permutation(rays.shape[0])])      # both kinds of rays in every wavefront, and among the first 1024
    n = rays.shape[0]
    assert n == 65536
    c = G.upload_case(tris); mem = c.mem
    d_rays = mem.upload(rays)
    exe = M.build_host(tmp_path)
    for compress in (False, True):
        grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=compress)
        got = run_multi(c, grid, d_rays, n, 8)
        want = M.host_walk(exe, tmp_path, grid.download(mem), tris, rays, 8)
        assert_lists(got, want["id"], want["t"], f"soup 100k compress={compress} against the host walk")
        if not compress:
            ids, t = M.lists_by_brute_force(tris, rays[:1024])
            assert_lists(got[:1024], ids, t, "soup 100k against the brute force")
            assert (ids >= 0).sum() > 1024
            hist = M.hit_histogram(want["id"])
            assert hist[0] > 0 and hist[8] > 0, "the batch has rays without a hit and rays with full lists"
        grid.free()
    mem.close()
