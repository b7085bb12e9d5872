"""Nearest-surface queries on the GPU (hagrid_amd/csrc/closest.hip): the device's answers against the fixture tests/golden/closest.npz (the whole 32-byte
record of every query, bit for bit) on Cell and SmallCell grids built on the device, with a traversal image present and ray binning on, before and after a
nearest-hit launch whose hints must not move; the counters against the host walk's totals; a larger live case against the host walk; torch tensors on
torch's stream; a MeshScene whose vertices are rewritten; edges and every argument error.
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import numpy as np
import pytest

import _closest as K
import _gpu_case as G
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu


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
    c = G.open_case(request.param, K.make_tris(request.param))
    c.queries = K.fixture_queries(c.tris)
    c.want = K.fixture_results(fixture, c.name)
    c.n = c.queries.shape[0]
    c.d_points = c.mem.upload(c.queries)
    yield c
    c.mem.close()


def run_closest(c, grid, d_points, n, counters=False, d_tris=None):
    """the answers of n queries as CLOSEST_DTYPE records (and the four counters), out of a poisoned buffer whose guard must stay untouched"""
    mem = c.mem
    d_res = P.alloc_out(mem, 32 * n)
    d_cnt = 0
    if counters:
        d_cnt = mem.alloc(32)
        mem.zero(d_cnt, 32)
    c.api.closest_points(grid, d_tris or c.d_tris, d_points, d_res, n, d_cnt)
    mem.synchronize()
    got = P.fetch(mem, d_res, c.api.CLOSEST_DTYPE, n).copy()
    mem.free(d_res)
    if counters:
        cnt = mem.download(d_cnt, np.int64, 4)
        mem.free(d_cnt)
        return got, cnt
    return got


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
    with G.image_present(c, grid):
        K.assert_results_equal(run_closest(c, grid, c.d_points, c.n), c.want, f"{c.name} image present")
        mem.set_ray_binning(1)
        K.assert_results_equal(run_closest(c, grid, c.d_points, c.n), c.want, f"{c.name} binning set")
    G.drop_image(c, grid)
    K.assert_results_equal(run_closest(c, grid, c.d_points, c.n), c.want, f"{c.name} traverse.image=0")
    mem.set_option("traverse.image", 2)


def test_no_interference_with_the_nearest_hit_path(case):
    """a nearest-hit launch, the queries, the launch again: the same hits, the hints kept for the ray buffer unchanged, the answers the fixture's"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    mem.set_option("traverse.image", 2)
    api.setup_traversal(grid)
    with G.nearest_hit_unmoved(c, grid):
        got = run_closest(c, grid, c.d_points, c.n)
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
    d_res = c.mem.alloc(32 * c.n)
    G.assert_totals_added(lambda d_cnt: c.api.closest_points(grid, c.d_tris, c.d_points, d_res, c.n, d_cnt), c.mem, cnt)
    c.mem.free(d_res)


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
    d_res = mem.alloc(32 * c.n + 64)
    d_cnt = mem.alloc(64)

    def call(g, tris, points, results, n, counters=0, flags=0):
        return L.hagrid_closest_points(mem._ctx, G.pod(g), G.vp(tris), G.vp(points), G.vp(results), n, G.vp(counters), flags)

    EINVAL = G.EINVAL
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
    assert L.hagrid_closest_points(None, G.pod(grid), G.vp(c.d_tris), G.vp(c.d_points), G.vp(d_res), c.n, None, 0) == EINVAL
    with pytest.raises(api.HagridError, match="aligned"):
        api.closest_points(grid, c.d_tris, c.d_points + 4, d_res, 8)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.closest_points(g2, c.d_tris, c.d_points, d_res, c.n)
            assert call(g2, c.d_tris, c.d_points, d_res, 0) == EINVAL
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
    c = G.upload_case(tris); mem = c.mem
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
    c = G.Case(); c.api, c.mem = api, mem
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
