"""Neighbour queries on the GPU (nearest_tris_kernel of hagrid_amd/csrc/closest.hip): the device's lists against the fixture tests/golden/nearest_k.npz
(entries bit for bit, records against the host walk's) on Cell and SmallCell grids built on the device, into poisoned and guarded buffers, with a traversal
image present, ray binning on and no image; no interference with the nearest-hit path; k = 1 against hagrid_closest_points in the same test; paging, ties
and labels with device cursors and labels; api.tris_within on torch tensors; counters against the host walk; batch shapes; the deep grids at every
stage; a live case; every argument error.
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import numpy as np
import pytest

import _closest as K
import _deep_grids as D
import _gpu_case as G
import _nearest_k as NK
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = G.EINVAL, G.ERANGE


@pytest.fixture(scope="module")
def fixture():
    return np.load(NK.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("nearest_k_host_gpu")
    return NK.build_host(d), d


@pytest.fixture(scope="module", params=K.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, the queries uploaded"""
    c = G.open_case(request.param, K.make_tris(request.param))
    c.queries = K.fixture_queries(c.tris)
    c.want, c.want_pages = NK.fixture_lists(fixture, c.name)
    c.n = c.queries.shape[0]
    c.d_points = c.mem.upload(c.queries)
    c.walk_records = {}
    yield c
    c.mem.close()


def run_nearest(api, mem, grid, d_tris, d_points, n, k, **kw):
    """NK.run_lists with hagrid_nearest_tris: (entries (n, k), records (n, k)[, the five counters])"""
    return NK.run_lists(api.nearest_tris, scene.CLOSEST_DTYPE, mem, grid, d_tris, d_points, n, k, **kw)


def want_records(c, host, compress):
    """the host walk's records at k = 8 over the device's grid (the CPU tests hold them to the numpy statement); the list for k is their first k"""
    if compress not in c.walk_records:
        exe, d = host
        e, r, _ = NK.host_walk(exe, d, c.grids[compress].download(c.mem), c.tris, c.queries, 8)
        NK.assert_lists_equal(e, c.want, f"{c.name}: the host walk over the device's grid against the fixture")
        c.walk_records[compress] = r
    return c.walk_records[compress]


def check_all_k(c, host, compress, what):
    grid = c.grids[compress]
    recs = want_records(c, host, compress)
    for k in (1, 2, 5, 8):
        e, r = run_nearest(c.api, c.mem, grid, c.d_tris, c.d_points, c.n, k)
        NK.assert_lists_equal(e, c.want[:, :k], f"{c.name} compress={compress} k={k} {what}: entries")
        NK.assert_lists_equal(r, recs[:, :k], f"{c.name} compress={compress} k={k} {what}: records")


@pytest.mark.parametrize("compress", [False, True])
def test_device_lists_equal_the_fixture(case, host, compress):
    """k in {1, 2, 5, 8}, entries and records, with the image present, with ray binning set, and with traverse.image = 0"""
    c = case; mem = c.mem
    grid = c.grids[compress]
    with G.image_present(c, grid):
        check_all_k(c, host, compress, "image present")
        mem.set_ray_binning(1)
        check_all_k(c, host, compress, "binning set")
    G.drop_image(c, grid)
    check_all_k(c, host, compress, "traverse.image=0")
    mem.set_option("traverse.image", 2)
    # entries alone, records alone
    e, _ = run_nearest(c.api, mem, grid, c.d_tris, c.d_points, c.n, 8, records=False)
    _, r = run_nearest(c.api, mem, grid, c.d_tris, c.d_points, c.n, 8, entries=False)
    NK.assert_lists_equal(e, c.want, "entries alone")
    NK.assert_lists_equal(r, want_records(c, host, compress), "records alone")


def test_no_interference_with_the_nearest_hit_path(case):
    """a nearest-hit launch, the queries, the launch again: the same hits, the hints kept for the ray buffer unchanged, the lists the fixture's"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    mem.set_option("traverse.image", 2)
    api.setup_traversal(grid)
    with G.nearest_hit_unmoved(c, grid):
        e, _ = run_nearest(api, mem, grid, c.d_tris, c.d_points, c.n, 8)
    NK.assert_lists_equal(e, c.want, f"{c.name} after a nearest-hit launch")


@pytest.mark.parametrize("compress", [False, True])
def test_k1_is_closest_points(case, compress):
    """both entry points in one test: entries are (d2, id) and records the whole 32 bytes of hagrid_closest_points, bit for bit"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[compress]
    d_res = P.alloc_out(mem, 32 * c.n)
    api.closest_points(grid, c.d_tris, c.d_points, d_res, c.n)
    mem.synchronize()
    want = P.fetch(mem, d_res, scene.CLOSEST_DTYPE, c.n).copy(); mem.free(d_res)
    e, r = run_nearest(api, mem, grid, c.d_tris, c.d_points, c.n, 1)
    K.assert_results_equal(r[:, 0], want, f"{c.name} compress={compress}: records at k = 1")
    assert (e["id"][:, 0] == want["id"]).all() and (K.bits(e["d2"][:, 0]) == K.bits(want["d2"])).all()
    assert (want["id"] >= 0).sum() > c.n // 2


def test_paging_ties_and_cursors(case):
    """the CPU cases on the device, cursors as device buffers: RADIUS and SPECIAL[32:48] paged to the end at k = 3 against scene.tris_within (and the lists
    do page); the first three pages of RADIUS, VERTEX and SPECIAL against the fixture -- on the mesh the boundaries fall inside ties; a cursor of d2 = -1
    excludes nothing, a NaN cursor everything"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[True]
    qs = c.queries[NK.PAGED]
    d_q = mem.upload(qs)

    def ask(which, cursors):
        d_w = mem.upload(np.ascontiguousarray(qs[which]))
        e, _ = run_nearest(api, mem, grid, c.d_tris, d_w, which.size, NK.PAGE_K, cursors=cursors, records=False)
        mem.free(d_w)
        return e

    lists, pages = NK.page_through(ask, qs.shape[0], NK.PAGE_K)
    NK.assert_pages_equal_csr(lists, scene.tris_within(c.tris, qs), c.name)
    two, four = {"soup": (300, 30), "mesh": (50, 30)}[c.name]
    assert (pages >= 2).sum() >= two and (pages >= 4).sum() >= four, "the lists must page"
    mem.free(d_q)
    qf = c.queries[NK.STORED]
    d_f = mem.upload(qf)
    got = NK.first_pages(lambda cursors: run_nearest(api, mem, grid, c.d_tris, d_f, qf.shape[0], NK.PAGE_K, cursors=cursors, records=False)[0], qf.shape[0])
    NK.assert_lists_equal(got.reshape(-1, NK.PAGE_K), c.want_pages.reshape(-1, NK.PAGE_K), f"{c.name}: pages against the fixture")
    if c.name == "mesh":
        first = got[0]                                         # VERTEX rows of STORED: 512 .. 704
        second = got[1]
        tie = (first["d2"][:, -1] == second["d2"][:, 0]) & (second["id"][:, 0] >= 0)
        assert tie[512:704].sum() >= 8 and (second["id"][tie, 0] > first["id"][tie, -1]).all(), "page boundaries inside ties"
    n = qf.shape[0]
    want8 = c.want[NK.STORED]
    for cid in (-1, 0, 2 ** 31 - 1):
        cur = NK.entries_of(np.full(n, -1.0, np.float32), np.full(n, cid, np.int32))
        NK.assert_lists_equal(run_nearest(api, mem, grid, c.d_tris, d_f, n, 8, cursors=cur, records=False)[0], want8, f"cursor (-1, {cid})")
    cur = NK.entries_of(np.full(n, np.nan, np.float32), np.full(n, -1, np.int32))
    e, r = run_nearest(api, mem, grid, c.d_tris, d_f, n, 8, cursors=cur)
    assert (e["id"] == -1).all() and (r["id"] == -1).all()
    active = qf[:, 3] >= 0
    assert (K.bits(e["d2"][active]) == K.bits(qf[active, 3] * qf[active, 3])[:, None]).all() and (e["d2"][~active] == -1).all()
    assert (K.bits(r["q"]) == K.bits(qf[:, None, 0:3])).all()
    mem.free(d_f)


def test_labels_on_the_meshs_own_vertices():
    """the stadium mesh, its vertices as queries, label = vertex index, triangle labels = its index triples, all on the device: the statement's lists;
    no list holds an incident triangle; labels of -1 skip nothing"""
    from hagrid_amd import api
    tris, F, q, labels = NK.stadium_labels()
    n = q.shape[0]
    mem = api.MemManager(keep=True)
    d_tris = mem.upload(tris); d_q = mem.upload(q); d_F = mem.upload(F)
    for compress in (False, True):
        grid = api.build_all(mem, d_tris, tris.shape[0], compress=compress)
        e, r = run_nearest(api, mem, grid, d_tris, d_q, n, 8, query_labels=labels, d_tri_labels=d_F)
        se, sr = scene.nearest_tris(tris, q, 8, query_labels=labels, tri_labels=F)
        NK.assert_lists_equal(e, se, f"labels compress={compress}: entries")
        NK.assert_lists_equal(r, sr, f"labels compress={compress}: records")
        assert not ((F[e["id"].clip(0)] == labels[:, None, None]).any(axis=2) & (e["id"] >= 0)).any()
        plain, _ = run_nearest(api, mem, grid, d_tris, d_q, n, 8, records=False)
        minus, _ = run_nearest(api, mem, grid, d_tris, d_q, n, 8, query_labels=np.full(n, -1, np.int32), d_tri_labels=d_F, records=False)
        NK.assert_lists_equal(minus, plain, "labels of -1 skip nothing")
        assert (plain["id"] != e["id"]).any() and (plain["d2"][:, 0] == 0).sum() > n // 2
        grid.free()
    mem.close()


def test_tris_within_on_torch_tensors(case):
    """api.tris_within with torch tensors on a torch stream against scene.tris_within, RADIUS section"""
    import torch
    c = case; api, mem = c.api, c.mem
    qs = np.ascontiguousarray(c.queries[K.RADIUS])
    want = scene.tris_within(c.tris, qs)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_pts = torch.from_numpy(qs).cuda()
            for k in (3, 8):
                got = api.tris_within(c.grids[True], c.d_tris, t_pts, k=k)
                off, ids, d2 = got["offsets"].cpu().numpy(), got["ids"].cpu().numpy(), got["d2"].cpu().numpy()
                assert (off == want["offsets"]).all() and (ids == want["ids"]).all() and (K.bits(d2) == K.bits(want["d2"])).all(), f"{c.name} k={k}"
                assert got["complete"] and got["pages"] == int(np.diff(want["offsets"]).max()) // k + 1
            # a bound on the pages: the lists are prefixes, and the answer says so
            got = api.tris_within(c.grids[True], c.d_tris, t_pts, k=3, max_pages=2)
            sizes = np.diff(got["offsets"].cpu().numpy())
            assert not got["complete"] and got["pages"] == 2 and (sizes == np.minimum(np.diff(want["offsets"]), 6)).all()
            stream.synchronize()
    finally:
        mem.use_stream(None)
    assert want["offsets"][-1] > qs.shape[0]


@pytest.mark.parametrize("compress", [False, True])
def test_counters_equal_the_host_walk(case, host, compress):
    c = case; api, mem = c.api, c.mem
    exe, d = host
    grid = c.grids[compress]
    for k in (1, 8):
        e, _, cnt = run_nearest(api, mem, grid, c.d_tris, c.d_points, c.n, k, counters=True, records=False)
        we, _, counts = NK.host_walk(exe, d, grid.download(mem), c.tris, c.queries, k)
        NK.assert_lists_equal(e, we, f"{c.name} compress={compress} k={k} against the host walk over the device's grid")
        assert cnt.tolist() == [c.n] + [int(counts[:, j].sum()) for j in range(4)]
        assert cnt[4] == (e["id"][:, k - 1] >= 0).sum() and 0 < cnt[4] < c.n and cnt[2] > 0 and cnt[3] > 0
    # the totals are ADDED: a second launch doubles them
    d_e = mem.alloc(8 * c.n * 8)
    G.assert_totals_added(lambda d_cnt: api.nearest_tris(grid, c.d_tris, c.d_points, c.n, 8, entries=d_e, counters=d_cnt), mem, cnt)
    mem.free(d_e)


def test_batch_shapes(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[True]
    # no points: nothing is launched, null buffers are fine
    api.nearest_tris(grid, c.d_tris, 0, 0, 8)
    api.nearest_tris(grid, 0, 0, 0, 1)
    for n, first in ((1, 0), (63, 5), (1000, 64), (65, 4031)):
        for k in (3, 8):
            e, r = run_nearest(api, mem, grid, c.d_tris, c.d_points + 16 * first, n, k)
            NK.assert_lists_equal(e, c.want[first:first + n, :k], f"{c.name} n={n} first={first} k={k}")
            assert (r["id"] == e["id"]).all() and (K.bits(r["d2"]) == K.bits(e["d2"])).all()


CASES = [(name, stage) for name in D.WALKED for stage in D.stages_of(name)]


@pytest.fixture(scope="module")
def deep_mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


@pytest.mark.parametrize("name,stage", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_deep_grids(deep_mem, host, name, stage):
    """every stage of every catalogue scene, k = 8, against the host brute force"""
    from hagrid_amd import api
    mem = deep_mem
    exe, d = host
    tris = D.make_tris(name)
    pts = D.points(tris)
    want_e, want_r = NK.host_brute(exe, d, tris, pts, 8)
    d_tris = mem.upload(tris); d_pts = mem.upload(pts)
    dev = D.DeviceStages(name, api, mem, d_tris, tris.shape[0])
    for st in D.STAGES[:D.STAGES.index(stage) + 1]:
        D.stage_grid(dev, st)
    e, r = run_nearest(api, mem, dev.grid, d_tris, d_pts, pts.shape[0], 8)
    NK.assert_lists_equal(e, want_e, f"{name} after {stage}: entries")
    NK.assert_lists_equal(r, want_r, f"{name} after {stage}: records")
    dev.grid.free(); mem.free(d_pts); mem.free(d_tris)


def test_live_case(tmp_path):
    """100 000 triangles, 16 384 queries (near the surface, uniform, uniform with r = 1 % of the diagonal, shuffled), k = 8: the device against the host walk
    over the SAME grid arrays (downloaded), counters included, and against the numpy statement for the first 256 queries"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    lo, hi = scene.tris_bbox(tris)
    diag = K.diagonal(lo, hi)
    n = 16384
    q = np.empty((n, 4), dtype=np.float32); q[:, 3] = np.inf
    q[:n // 2, 0:3] = K.near_surface_points(tris, lo, hi, n // 2, 11)
    q[n // 2:, 0:3] = K.uniform_points(lo, hi, n // 2, 12)
    q[3 * n // 4:, 3] = np.float32(0.01) * diag
    q = np.ascontiguousarray(q[np.random.default_rng(5).permutation(n)])
    c = G.upload_case(tris); mem, d_tris = c.mem, c.d_tris
    d_pts = mem.upload(q)
    exe = NK.build_host(tmp_path)
    for compress in (False, True):
        grid = api.build_all(mem, d_tris, tris.shape[0], compress=compress)
        e, r, cnt = run_nearest(api, mem, grid, d_tris, d_pts, n, 8, counters=True)
        we, wr, counts = NK.host_walk(exe, tmp_path, grid.download(mem), tris, q, 8)
        NK.assert_lists_equal(e, we, f"soup 100k compress={compress} against the host walk: entries")
        NK.assert_lists_equal(r, wr, f"soup 100k compress={compress} against the host walk: records")
        assert cnt.tolist() == [n] + [int(counts[:, j].sum()) for j in range(4)]
        if not compress:
            se, sr = scene.nearest_tris(tris, q[:256], 8)
            NK.assert_lists_equal(e[:256], se, "soup 100k against the statement: entries")
            NK.assert_lists_equal(r[:256], sr, "soup 100k against the statement: records")
            assert 0 < cnt[4] < n and (we["id"][:, 0] < 0).any()
            assert counts[:, 1].mean() < tris.shape[0] / 10
        grid.free()
    mem.close()


def test_errors_leave_the_context_working(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    n = c.n
    d_e = mem.alloc(8 * n * 8 + 64); d_r = mem.alloc(32 * n * 8 + 64); d_cnt = mem.alloc(64)
    d_cur = mem.alloc(8 * n + 64); d_ql = mem.alloc(4 * n + 64); d_tl = mem.alloc(12 * c.tris.shape[0] + 64)
    mem.zero(d_cur, 8 * n + 64); mem.zero(d_ql, 4 * n + 64); mem.zero(d_tl, 12 * c.tris.shape[0] + 64)
    vp = G.vp

    def call(g=grid, tris=c.d_tris, points=c.d_points, num=n, k=8, cursors=0, ql=0, tl=0, entries=d_e, records=d_r, counters=0, flags=0):
        return L.hagrid_nearest_tris(mem._ctx, G.pod(g), vp(tris), vp(points), num, k, vp(cursors), vp(ql), vp(tl), vp(entries), vp(records),
                                     vp(counters), flags)

    assert call(counters=d_cnt, cursors=d_cur, ql=d_ql, tl=d_tl) == 0
    assert call(g=None) == EINVAL and call(tris=0) == EINVAL and call(points=0) == EINVAL and call(num=-1) == EINVAL
    for k in (0, -1, 9, 1 << 20):
        assert call(k=k) == EINVAL
    for flags in (1, 2, 1 << 31):
        assert call(flags=flags) == EINVAL
        assert b"flag" in L.hagrid_last_error(mem._ctx)
    assert call(entries=0, records=0) == EINVAL
    assert call(entries=0) == 0 and call(records=0) == 0
    assert call(ql=d_ql) == EINVAL and call(tl=d_tl) == EINVAL
    assert call(tris=c.d_tris + 4) == EINVAL and call(points=c.d_points + 8, num=n - 1) == EINVAL
    assert call(entries=d_e + 4) == EINVAL and call(records=d_r + 8) == EINVAL and call(cursors=d_cur + 4) == EINVAL
    assert call(ql=d_ql + 2, tl=d_tl) == EINVAL and call(ql=d_ql, tl=d_tl + 2) == EINVAL and call(counters=d_cnt + 4) == EINVAL
    assert call(num=(1 << 31) // 8 + 1, k=8) == ERANGE and call(num=2 ** 31 - 1, k=2) == ERANGE
    assert call(num=0, tris=0, points=0, entries=0, records=0) == 0
    assert L.hagrid_nearest_tris(None, G.pod(grid), vp(c.d_tris), vp(c.d_points), n, 8, None, None, None, vp(d_e), None, None, 0) == EINVAL
    with pytest.raises(api.HagridError, match="aligned"):
        api.nearest_tris(grid, c.d_tris, c.d_points + 4, 8, 8, entries=d_e)
    # a grid given up for traversal has no construction format left; a bad shift
    g2 = api.build_all(mem, c.d_tris, c.tris.shape[0])
    shift = g2.pod.shift
    g2.pod.shift = 16
    assert call(g=g2) == EINVAL and b"shift" in L.hagrid_last_error(mem._ctx)
    g2.pod.shift = shift
    with G.released_grid(c, g2) as released:
        if released is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.nearest_tris(g2, c.d_tris, c.d_points, n, 8, entries=d_e)
            assert call(g=g2, num=0) == EINVAL
    for p in (d_e, d_r, d_cnt, d_cur, d_ql, d_tl):
        mem.free(p)
    api.setup_traversal(grid)
    e, _ = run_nearest(api, mem, grid, c.d_tris, c.d_points, n, 8, records=False)
    NK.assert_lists_equal(e, c.want, f"{c.name} after the refused calls")
