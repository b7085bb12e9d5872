"""Nearest-surface queries on the GPU (hagrid_amd/csrc/closest.hip): the device's answers against the fixture tests/golden/closest.npz (the whole 32-byte
record of every query, bit for bit) on Cell and SmallCell grids built on the device, with a traversal image present and ray binning on, before and after a
nearest-hit launch whose hints must not move; the counters against the host walk's totals; a larger live case against the host walk; torch tensors on
torch's stream; a MeshScene whose vertices are rewritten; edges and every argument error."""
import numpy as np
import pytest

import _closest as K
from hagrid_amd import scene

pytestmark = pytest.mark.gpu


class Case:
    pass


@pytest.fixture(scope="module")
def fixture():
    return np.load(K.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("closest_host_gpu")
    return K.build_host(d), d


@pytest.fixture(scope="module", params=K.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, the queries uploaded"""
    from hagrid_amd import api
    c = Case()
    c.api, c.name = api, request.param
    c.tris = K.make_tris(c.name)
    c.mem = api.MemManager(keep=True)
    c.d_tris = c.mem.upload(c.tris)
    c.grids = {False: api.build_all(c.mem, c.d_tris, c.tris.shape[0]), True: api.build_all(c.mem, c.d_tris, c.tris.shape[0], compress=True)}
    assert c.grids[True].small_cells and not c.grids[False].small_cells
    c.queries = K.fixture_queries(c.tris)
    c.want = K.fixture_results(fixture, c.name)
    c.n = c.queries.shape[0]
    c.d_points = c.mem.upload(c.queries)
    yield c
    c.mem.close()


def run_closest(c, grid, d_points, n, counters=False, pad=4, d_tris=None):
    """the answers of n queries as CLOSEST_DTYPE records (and the four counters); the buffer is `pad` records longer and those must stay untouched"""
    mem = c.mem
    d_res = mem.alloc(32 * (n + pad))
    mem.one(d_res, 32 * (n + pad))
    d_cnt = 0
    if counters:
        d_cnt = mem.alloc(32)
        mem.zero(d_cnt, 32)
    c.api.closest_points(grid, d_tris or c.d_tris, d_points, d_res, n, d_cnt)
    mem.synchronize()
    got = mem.download(d_res, c.api.CLOSEST_DTYPE, n + pad)
    mem.free(d_res)
    assert (got[n:].view(np.uint32) == 0xFFFFFFFF).all(), "written beyond num_points records"
    if counters:
        cnt = mem.download(d_cnt, np.int64, 4)
        mem.free(d_cnt)
        return got[:n], cnt
    return got[:n]


@pytest.mark.parametrize("compress", [False, True])
def test_device_results_equal_the_fixture(case, compress):
    c = case
    c.mem.set_option("traverse.image", 0)
    got = run_closest(c, c.grids[compress], c.d_points, c.n)
    K.assert_results_equal(got, c.want, f"{c.name} compress={compress}")
    c.mem.set_option("traverse.image", 2)


@pytest.mark.parametrize("compress", [False, True])
def test_image_and_ray_binning_are_ignored(case, compress):
    c = case; mem = c.mem
    grid = c.grids[compress]
    mem.set_option("traverse.image", 2)
    c.api.setup_traversal(grid)
    assert mem.image_bytes(grid) > 0
    try:
        K.assert_results_equal(run_closest(c, grid, c.d_points, c.n), c.want, f"{c.name} image present")
        mem.set_ray_binning(1)
        K.assert_results_equal(run_closest(c, grid, c.d_points, c.n), c.want, f"{c.name} binning set")
    finally:
        mem.set_ray_binning(0)
    assert mem.image_bytes(grid) > 0, "the query dropped the traversal image"
    mem.set_option("traverse.image", 0)
    c.api.setup_traversal(grid)
    assert mem.image_bytes(grid) == 0
    K.assert_results_equal(run_closest(c, grid, c.d_points, c.n), c.want, f"{c.name} traverse.image=0")
    mem.set_option("traverse.image", 2)


def test_no_interference_with_the_nearest_hit_path(case):
    """a nearest-hit launch, the queries, the launch again: the same hits, the hints kept for the ray buffer unchanged, the answers the fixture's"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    mem.set_option("traverse.image", 2)
    api.setup_traversal(grid)
    rays = scene.make_rays_primary(grid.bbox_min, grid.bbox_max, 64, 64)
    nr = rays.shape[0]
    d_rays = mem.upload(rays)
    d_hits = mem.alloc(16 * nr)

    def nearest():
        mem.one(d_hits, 16 * nr)
        api.traverse_grid(grid, c.d_tris, d_rays, d_hits, nr)
        mem.synchronize()
        return mem.download(d_hits, api.HIT_DTYPE, nr)

    before = nearest()
    state = mem.order_state(d_rays)
    got = run_closest(c, grid, c.d_points, c.n)
    assert mem.order_state(d_rays) == state, "the hints of the nearest-hit path moved"
    after = nearest()
    mem.free(d_hits); mem.free(d_rays)
    assert (before.view(np.uint32) == after.view(np.uint32)).all() and (before["id"] >= 0).any()
    K.assert_results_equal(got, c.want, f"{c.name} after a nearest-hit launch")


@pytest.mark.parametrize("compress", [False, True])
def test_counters_equal_the_host_walk(case, host, compress):
    c = case
    exe, d = host
    grid = c.grids[compress]
    got, cnt = run_closest(c, grid, c.d_points, c.n, counters=True)
    want, counts = K.host_walk(exe, d, grid.download(c.mem), c.tris, c.queries)
    K.assert_results_equal(got, want, f"{c.name} compress={compress} against the host walk over the device's grid")
    assert cnt.tolist() == [c.n, int(counts[:, 0].sum()), int(counts[:, 1].sum()), int(counts[:, 2].sum())]
    assert cnt[2] > 0 and cnt[3] > 0
    # the totals are ADDED: a second launch doubles them
    mem = c.mem
    d_res = mem.alloc(32 * c.n); d_cnt = mem.upload(cnt)
    c.api.closest_points(grid, c.d_tris, c.d_points, d_res, c.n, d_cnt)
    mem.synchronize()
    assert (mem.download(d_cnt, np.int64, 4) == 2 * cnt).all()
    mem.free(d_res); mem.free(d_cnt)


def test_edges(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[True]
    # no points: nothing is launched, null buffers are fine
    api.closest_points(grid, c.d_tris, 0, 0, 0)
    api.closest_points(grid, 0, 0, 0, 0, 0)
    # batches that are not a multiple of 64, at an offset into the point buffer
    for n, first in ((1, 0), (63, 5), (1000, 64), (4095, 1), (65, 4031)):
        got = run_closest(c, grid, c.d_points + 16 * first, n)
        K.assert_results_equal(got, c.want[first:first + n], f"{c.name} n={n} first={first}")


def test_errors_leave_the_context_working(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    import ctypes as C
    d_res = mem.alloc(32 * c.n + 64)
    d_cnt = mem.alloc(64)

    def call(g, tris, points, results, n, counters=0, flags=0):
        return L.hagrid_closest_points(mem._ctx, C.byref(g.pod) if g is not None else None, C.c_void_p(tris), C.c_void_p(points), C.c_void_p(results), n, C.c_void_p(counters), flags)

    EINVAL = -1
    assert call(grid, c.d_tris, c.d_points, d_res, c.n, d_cnt) == 0
    assert call(None, c.d_tris, c.d_points, d_res, c.n) == EINVAL
    assert call(grid, 0, c.d_points, d_res, c.n) == EINVAL and call(grid, c.d_tris, 0, d_res, c.n) == EINVAL and call(grid, c.d_tris, c.d_points, 0, c.n) == EINVAL
    assert call(grid, c.d_tris + 4, c.d_points, d_res, c.n) == EINVAL
    assert call(grid, c.d_tris, c.d_points + 8, d_res, c.n - 1) == EINVAL
    assert call(grid, c.d_tris, c.d_points, d_res + 8, c.n) == EINVAL and call(grid, c.d_tris, c.d_points, d_res + 4, c.n) == EINVAL
    assert call(grid, c.d_tris, c.d_points, d_res, c.n, d_cnt + 4) == EINVAL
    for flags in (1, 2, 4, 1 << 31):
        assert call(grid, c.d_tris, c.d_points, d_res, c.n, 0, flags) == EINVAL
        assert b"flag" in L.hagrid_last_error(mem._ctx)
    assert call(grid, c.d_tris, c.d_points, d_res, -1) == EINVAL
    assert L.hagrid_closest_points(None, C.byref(grid.pod), C.c_void_p(c.d_tris), C.c_void_p(c.d_points), C.c_void_p(d_res), c.n, None, 0) == EINVAL
    with pytest.raises(api.HagridError, match="aligned"):
        api.closest_points(grid, c.d_tris, c.d_points + 4, d_res, 8)
    # a grid given up for traversal has no construction format left
    g2 = api.build_all(mem, c.d_tris, c.tris.shape[0])
    mem.set_option("traverse.image", 2)
    api.setup_traversal(g2)
    if mem.image_bytes(g2) > 0:
        api.release_for_traversal(g2)
        with pytest.raises(api.HagridError, match="released"):
            api.closest_points(g2, c.d_tris, c.d_points, d_res, c.n)
        assert call(g2, c.d_tris, c.d_points, d_res, 0) == EINVAL
    g2.free()
    mem.free(d_res); mem.free(d_cnt)
    api.setup_traversal(grid)
    K.assert_results_equal(run_closest(c, grid, c.d_points, c.n), c.want, f"{c.name} after the refused calls")


def test_torch_tensors_on_torchs_stream(case):
    """points and results are torch tensors, the launch runs on a torch stream between torch work that writes the points and torch work that reads the results"""
    import torch
    c = case; api, mem = c.api, c.mem
    host_pts = torch.from_numpy(c.queries.copy())
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_pts = torch.zeros((c.n, 4), dtype=torch.float32, device="cuda")
            t_pts.copy_(host_pts, non_blocking=False)
            t_res = torch.full((c.n, 8), -1, dtype=torch.int32, device="cuda")
            t_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            api.closest_points(c.grids[True], c.d_tris, t_pts.data_ptr(), t_res.data_ptr(), c.n, t_cnt.data_ptr())
            found = (t_res[:, 4] >= 0).sum()                     # torch work on the same stream, after the launch
            res = t_res.cpu().numpy(); cnt = t_cnt.cpu().numpy()
            stream.synchronize()
    finally:
        mem.use_stream(None)
    got = np.ascontiguousarray(res).view(scene.CLOSEST_DTYPE).reshape(-1)
    K.assert_results_equal(got, c.want, f"{c.name} torch tensors")
    assert int(found) == int((c.want["id"] >= 0).sum()) and cnt[0] == c.n and cnt[2] > 0


def test_larger_live_case(tmp_path):
    """100 000 triangles, 65 536 queries (near the surface, uniform with and without a radius, in one shuffled batch): the device's answers against the host
    walk over the SAME grid arrays (downloaded), counters included, and against the numpy statement for the first 256 queries"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    lo, hi = scene.tris_bbox(tris)
    diag = K.diagonal(lo, hi)
    q = np.empty((65536, 4), dtype=np.float32); q[:, 3] = np.inf
    q[:32768, 0:3] = K.near_surface_points(tris, lo, hi, 32768, 11)
    q[32768:, 0:3] = K.uniform_points(lo, hi, 32768, 12)
    q[49152:, 3] = np.float32(0.01) * diag
    q = np.ascontiguousarray(q[np.random.default_rng(5).permutation(q.shape[0])])
    n = q.shape[0]
    mem = api.MemManager(keep=True)
    c = Case(); c.api, c.mem = api, mem
    c.d_tris = mem.upload(tris)
    d_pts = mem.upload(q)
    exe = K.build_host(tmp_path)
    for compress in (False, True):
        grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=compress)
        got, cnt = run_closest(c, grid, d_pts, n, counters=True)
        want, counts = K.host_walk(exe, tmp_path, grid.download(mem), tris, q)
        K.assert_results_equal(got, want, f"soup 100k compress={compress} against the host walk")
        assert cnt.tolist() == [n, int(counts[:, 0].sum()), int(counts[:, 1].sum()), int(counts[:, 2].sum())]
        if not compress:
            K.assert_results_equal(got[:256], scene.closest_points(tris, q[:256]), "soup 100k against the statement")
            assert (want["id"] >= 0).sum() > n // 2 and (want["id"] < 0).any(), "the batch has queries that find nothing within their radius"
            assert counts[:, 1].mean() < tris.shape[0] / 10
        grid.free()
    mem.close()


def test_rebuild_after_vertices_were_rewritten():
    """the frame loop of api.MeshScene: assemble -> build -> query, then torch rewrites the vertices in place, assemble -> build -> query again: every
    answer is the statement's on the triangles of that frame (a bad index makes a triangle without a surface, which no query returns)"""
    import torch
    from hagrid_amd import api
    V, F = scene.make_stadium_mesh(0.05)
    V = np.ascontiguousarray(V, np.float32); F = np.ascontiguousarray(F, np.int32).copy()
    F[7] = (0, 1, V.shape[0] + 5)                                # a bad index: the degenerate triangle on vertex 0
    nt = F.shape[0]
    mem = api.MemManager(keep=True)
    c = Case(); c.api, c.mem = api, mem
    tV = torch.from_numpy(V).cuda(); tF = torch.from_numpy(F).cuda()
    torch.cuda.synchronize()
    ms = api.MeshScene(mem, [(tV.data_ptr(), V.shape[0], tF.data_ptr(), nt)])
    d_tris = mem.alloc(48 * nt)
    for frame in range(2):
        if frame == 1:
            V = (V * np.float32([1.0, 1.25, 0.8]) + np.float32(0.05) * np.sin(3.0 * V[:, [1, 2, 0]]).astype(np.float32)).astype(np.float32)
            tV.copy_(torch.from_numpy(V)); torch.cuda.synchronize()
        ms.assemble(0, d_tris)
        grid = api.build_all(mem, d_tris, nt)
        mem.synchronize()
        tris = mem.download(d_tris, np.float32, 12 * nt).reshape(nt, 12)
        assert (tris[7, [3, 7, 11]] == 0).all()
        lo, hi = scene.tris_bbox(tris)
        q = np.empty((1024, 4), dtype=np.float32); q[:, 3] = np.inf
        q[:512, 0:3] = K.near_surface_points(tris, lo, hi, 512, 21 + frame)
        q[512:, 0:3] = K.uniform_points(lo, hi, 512, 31 + frame); q[768:, 3] = np.float32(0.03) * K.diagonal(lo, hi)
        q[0, 0:3] = tris[7, 0:3]                                  # on the degenerate triangle
        d_pts = mem.upload(q)
        got = run_closest(c, grid, d_pts, q.shape[0], d_tris=d_tris)
        K.assert_results_equal(got, scene.closest_points(tris, q), f"frame {frame}")
        assert (got["id"] != 7).all() and (got["id"] >= 0).sum() > 768
        mem.free(d_pts); grid.free()
    assert ms.bad_indices() == 2
    ms.close(); mem.free(d_tris); mem.close()
