"""Capsule queries on the GPU (segment_tris_kernel, hagrid_amd/csrc/capsule.hip): the device's lists against the fixture
tests/golden/segments.npz (entries bit for bit, records against the host walk's) on Cell and SmallCell grids built on the device, into poisoned and
guarded buffers, with a traversal image present, ray binning on and no image; no interference with the nearest-hit path; a == b against
hagrid_nearest_tris and hagrid_closest_points in the same test; paging, ties and labels with device cursors and labels; api.tris_near_segments on torch
tensors; counters against the host walk; batch shapes; the deep grids at every stage; a live case; every argument error.
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import numpy as np
import pytest

import _closest as K
import _deep_grids as D
import _gpu_case as G
import _nearest_k as NK
import _poison as P
import _segments as SG
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = G.EINVAL, G.ERANGE


@pytest.fixture(scope="module")
def fixture():
    return np.load(SG.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("segments_host_gpu")
    return SG.build_host(d), d


@pytest.fixture(scope="module", params=K.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, the segments and the labels uploaded"""
    c = G.open_case(request.param, K.make_tris(request.param))
    c.segments = SG.fixture_segments(c.tris, c.name)
    c.tl, own = SG.fixture_labels(c.name, c.tris)
    c.ql = SG.fixture_query_labels(own)
    c.want, c.want_pages = SG.fixture_lists(fixture, c.name)
    c.n = c.segments.shape[0]
    c.d_segments = c.mem.upload(c.segments)
    c.d_ql = c.mem.upload(c.ql)
    c.d_tl = c.mem.upload(c.tl)
    c.walk_records = {}
    yield c
    c.mem.close()


def run_segments(api, mem, grid, d_tris, d_segments, n, k, **kw):
    """NK.run_lists with hagrid_segment_tris: (entries (n, k), records (n, k)[, the five counters])"""
    return NK.run_lists(api.segment_tris, SG.RECORD, mem, grid, d_tris, d_segments, n, k, **kw)


def run_fixture(c, grid, k, **kw):
    return run_segments(c.api, c.mem, grid, c.d_tris, c.d_segments, c.n, k, d_query_labels=c.d_ql, d_tri_labels=c.d_tl, **kw)


def want_records(c, host, compress):
    """the host walk's records at k = 8 over the device's grid (the CPU tests hold them to the numpy statement); the list for k is their first k"""
    if compress not in c.walk_records:
        exe, d = host
        e, r, _ = SG.host_walk(exe, d, c.grids[compress].download(c.mem), c.tris, c.segments, 8, query_labels=c.ql, tri_labels=c.tl)
        NK.assert_lists_equal(e, c.want, f"{c.name}: the host walk over the device's grid against the fixture")
        c.walk_records[compress] = r
    return c.walk_records[compress]


def check_all_k(c, host, compress, what, ks=(1, 2, 5, 8)):
    grid = c.grids[compress]
    recs = want_records(c, host, compress)
    for k in ks:
        e, r = run_fixture(c, grid, k)
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
        check_all_k(c, host, compress, "binning set", ks=(3, 8))
    G.drop_image(c, grid)
    check_all_k(c, host, compress, "traverse.image=0", ks=(1, 8))
    mem.set_option("traverse.image", 2)
    # entries alone, records alone
    e, _ = run_fixture(c, grid, 8, records=False)
    _, r = run_fixture(c, grid, 8, entries=False)
    NK.assert_lists_equal(e, c.want, "entries alone")
    NK.assert_lists_equal(r, want_records(c, host, compress), "records alone")


def test_no_interference_with_the_nearest_hit_path(case):
    """a nearest-hit launch, the queries, the launch again: the same hits, the hints kept for the ray buffer unchanged, the lists the fixture's"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    mem.set_option("traverse.image", 2)
    api.setup_traversal(grid)
    with G.nearest_hit_unmoved(c, grid):
        e, _ = run_fixture(c, grid, 8)
    NK.assert_lists_equal(e, c.want, f"{c.name} after a nearest-hit launch")


@pytest.mark.parametrize("compress", [False, True])
def test_zero_length_is_nearest_tris_and_closest_points(case, compress):
    """the three entry points in one test, on the ZERO section (a == b): with the first label of each pair (second -1) entries and records are
    hagrid_nearest_tris' for the points (a, r), bit for bit, at k = 1 and 8; at k = 1 without labels they are hagrid_closest_points' output"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[compress]
    z = np.ascontiguousarray(c.segments[SG.ZERO]); n = z.shape[0]
    pts = np.ascontiguousarray(z[:, 0:4])
    d_z = mem.upload(z); d_p = mem.upload(pts)
    rng = np.random.default_rng(3)
    tl = rng.integers(0, 64, (c.tris.shape[0], 3)).astype(np.int32)
    ql = rng.integers(-1, 64, n).astype(np.int32)
    d_tl = mem.upload(tl); d_ql = mem.upload(ql)
    for k in (1, 8):
        for labelled in (False, True):
            d_e = P.alloc_out(mem, 8 * n * k); d_r = P.alloc_out(mem, 32 * n * k)
            api.nearest_tris(grid, c.d_tris, d_p, n, k, entries=d_e, records=d_r, query_labels=d_ql if labelled else 0, tri_labels=d_tl if labelled else 0)
            mem.synchronize()
            pe = P.fetch(mem, d_e, SG.ENTRY, n * k).reshape(n, k).copy(); pr = P.fetch(mem, d_r, scene.CLOSEST_DTYPE, n * k).reshape(n, k).copy()
            mem.free(d_e); mem.free(d_r)
            e, r = run_segments(api, mem, grid, c.d_tris, d_z, n, k, query_labels=np.stack([ql, np.full_like(ql, -1)], axis=1) if labelled else None, d_tri_labels=d_tl)
            NK.assert_lists_equal(e, pe, f"{c.name} compress={compress} k={k} labelled={labelled}: entries against hagrid_nearest_tris")
            NK.assert_lists_equal(r.view(scene.CLOSEST_DTYPE), pr, f"{c.name} compress={compress} k={k} labelled={labelled}: records against hagrid_nearest_tris")
            assert not labelled or (e["id"] != e0["id"]).any()
            e0 = e
    d_res = P.alloc_out(mem, 32 * n)
    api.closest_points(grid, c.d_tris, d_p, d_res, n)
    mem.synchronize()
    want = P.fetch(mem, d_res, scene.CLOSEST_DTYPE, n).copy(); mem.free(d_res)
    e, r = run_segments(api, mem, grid, c.d_tris, d_z, n, 1)
    K.assert_results_equal(r[:, 0].view(scene.CLOSEST_DTYPE), want, f"{c.name} compress={compress}: records at k = 1 against hagrid_closest_points")
    assert (e["id"][:, 0] == want["id"]).all() and (K.bits(e["d2"][:, 0]) == K.bits(want["d2"])).all() and (want["id"] >= 0).sum() > n // 2
    for p in (d_z, d_p, d_tl, d_ql):
        mem.free(p)


def test_paging_ties_and_cursors(case):
    """the CPU cases on the device, cursors and labels as device buffers: every fourth segment with a finite radius (the labelled ones among them) paged to
    its end at k = 3 against scene.tris_near_segments, and the lists do page; the first three pages against the fixture; page boundaries inside ties; a cursor
    of d2 = -1 excludes nothing, a NaN cursor everything"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[True]
    ss, sl = c.segments[SG.PAGED[::4]], c.ql[SG.PAGED[::4]]          # a quarter of what the CPU test pages: every family, the labelled one at the end

    def ask(which, cursors):
        d_w = mem.upload(np.ascontiguousarray(ss[which]))
        e, _ = run_segments(api, mem, grid, c.d_tris, d_w, which.size, SG.PAGE_K, cursors=cursors, query_labels=sl[which], d_tri_labels=c.d_tl, records=False)
        mem.free(d_w)
        return e

    lists, pages = NK.page_through(ask, ss.shape[0], SG.PAGE_K, max_pages=256)
    NK.assert_pages_equal_csr(lists, scene.tris_near_segments(c.tris, ss, query_labels=sl, tri_labels=c.tl), c.name)
    assert (pages >= 2).sum() >= 120 and (pages >= 4).sum() >= 75 and (pages[-64:] >= 2).sum() >= 16, "the lists must page"
    sf = np.ascontiguousarray(c.segments[SG.STORED]); n = sf.shape[0]
    d_f = mem.upload(sf); d_fl = mem.upload(np.ascontiguousarray(c.ql[SG.STORED]))
    kw = dict(d_query_labels=d_fl, d_tri_labels=c.d_tl)
    got = NK.first_pages(lambda cursors: run_segments(api, mem, grid, c.d_tris, d_f, n, SG.PAGE_K, cursors=cursors, records=False, **kw)[0], n)
    NK.assert_lists_equal(got.reshape(-1, SG.PAGE_K), c.want_pages.reshape(-1, SG.PAGE_K), f"{c.name}: pages against the fixture")
    first, second = got[0], got[1]
    tie = (first["d2"][:, -1] == second["d2"][:, 0]) & (second["id"][:, 0] >= 0)
    assert (second["id"][tie, 0] > first["id"][tie, -1]).all()
    if c.name == "mesh":
        assert tie.sum() >= 8, "page boundaries inside ties"
    want8 = c.want[SG.STORED]
    for cid in (-1, 0, 2 ** 31 - 1):
        cur = NK.entries_of(np.full(n, -1.0, np.float32), np.full(n, cid, np.int32))
        NK.assert_lists_equal(run_segments(api, mem, grid, c.d_tris, d_f, n, 8, cursors=cur, records=False, **kw)[0], want8, f"cursor (-1, {cid})")
    cur = NK.entries_of(np.full(n, np.nan, np.float32), np.full(n, -1, np.int32))
    e, r = run_segments(api, mem, grid, c.d_tris, d_f, n, 8, cursors=cur, **kw)
    assert (e["id"] == -1).all() and (r["id"] == -1).all()
    assert (K.bits(e["d2"]) == K.bits(sf[:, 3] * sf[:, 3])[:, None]).all()
    assert (K.bits(r["q"]) == K.bits(sf[:, None, 0:3])).all() and (K.bits(r["s"]) == 0).all()
    mem.free(d_f); mem.free(d_fl)


def test_labels_on_the_meshs_own_edges(host):
    """the stadium mesh, its own edges as segments, labels = the edges' vertex pairs, triangle labels = its index triples, all on the device: the host brute
    force's lists; no list holds a triangle that shares a vertex with the edge; labels of -1 skip nothing; MeshScene.edge_labels gives the same edges"""
    from hagrid_amd import api
    exe, d = host
    tris, F, s, labels = SG.edge_labels_case()
    n = s.shape[0]
    mem = api.MemManager(keep=True)
    d_tris = mem.upload(tris); d_s = mem.upload(s); d_F = mem.upload(F)
    we, wr = SG.host_brute(exe, d, tris, s, 8, query_labels=labels, tri_labels=F)
    for compress in (False, True):
        grid = api.build_all(mem, d_tris, tris.shape[0], compress=compress)
        e, r = run_segments(api, mem, grid, d_tris, d_s, n, 8, query_labels=labels, d_tri_labels=d_F)
        NK.assert_lists_equal(e, we, f"labels compress={compress}: entries")
        NK.assert_lists_equal(r, wr, f"labels compress={compress}: records")
        assert not (((F[e["id"].clip(0)][:, :, :, None] == labels[:, None, None, :]).any(axis=(2, 3))) & (e["id"] >= 0)).any()
        plain, _ = run_segments(api, mem, grid, d_tris, d_s, n, 8, records=False)
        minus, _ = run_segments(api, mem, grid, d_tris, d_s, n, 8, query_labels=np.full((n, 2), -1, np.int32), d_tri_labels=d_F, records=False)
        NK.assert_lists_equal(minus, plain, "labels of -1 skip nothing")
        assert (plain["id"] != e["id"]).any()
        grid.free()
    V = np.ascontiguousarray(scene.make_stadium_mesh(0.05)[0], np.float32)
    d_V = mem.upload(V)
    ms = api.MeshScene(mem, [(d_V, V.shape[0], d_F, F.shape[0])])
    pairs, lab = ms.edge_labels()
    mem.synchronize()
    import torch
    stream = torch.cuda.Stream()
    try:
        mem.use_stream(stream.cuda_stream)                      # the manager on a stream that is not torch's current one
        pairs2, lab2 = ms.edge_labels()
        mem.synchronize()
    finally:
        mem.use_stream(None)
    assert (pairs2.cpu().numpy() == scene.mesh_edges(F)).all() and (lab2.cpu().numpy() == scene.mesh_edges(F)).all()
    assert (lab.cpu().numpy() == scene.mesh_edges(F)).all() and (pairs.cpu().numpy() == scene.mesh_edges(F)).all()
    mem.close()


def test_tris_near_segments_on_torch_tensors(case):
    """api.tris_near_segments with torch tensors on a torch stream against scene.tris_near_segments: a quarter of the SHORT_R section, and of the labelled OWN section"""
    import torch
    c = case; api, mem = c.api, c.mem
    qs = np.ascontiguousarray(c.segments[SG.SHORT_R][::4])
    want = scene.tris_near_segments(c.tris, qs)
    own = np.ascontiguousarray(c.segments[SG.OWN][::4]); own_l = np.ascontiguousarray(c.ql[SG.OWN][::4])
    want_own = scene.tris_near_segments(c.tris, own, query_labels=own_l, tri_labels=c.tl)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_s = torch.from_numpy(qs).cuda()
            for k in (3, 8):
                got = api.tris_near_segments(c.grids[True], c.d_tris, t_s, k=k)
                off, ids, d2 = got["offsets"].cpu().numpy(), got["ids"].cpu().numpy(), got["d2"].cpu().numpy()
                assert (off == want["offsets"]).all() and (ids == want["ids"]).all() and (K.bits(d2) == K.bits(want["d2"])).all(), f"{c.name} k={k}"
                assert got["complete"] and got["pages"] == int(np.diff(want["offsets"]).max()) // k + 1
            got = api.tris_near_segments(c.grids[True], c.d_tris, t_s, k=3, max_pages=2)
            sizes = np.diff(got["offsets"].cpu().numpy())
            assert not got["complete"] and got["pages"] == 2 and (sizes == np.minimum(np.diff(want["offsets"]), 6)).all()
            got = api.tris_near_segments(c.grids[True], c.d_tris, torch.from_numpy(own).cuda(), k=8, query_labels=torch.from_numpy(own_l).cuda(), tri_labels=c.d_tl)
            assert (got["offsets"].cpu().numpy() == want_own["offsets"]).all() and (got["ids"].cpu().numpy() == want_own["ids"]).all()
            assert (K.bits(got["d2"].cpu().numpy()) == K.bits(want_own["d2"])).all()
            stream.synchronize()
    finally:
        mem.use_stream(None)
    assert want["offsets"][-1] > qs.shape[0] and want_own["offsets"][-1] > own.shape[0]


@pytest.mark.parametrize("compress", [False, True])
def test_counters_equal_the_host_walk(case, host, compress):
    c = case; api, mem = c.api, c.mem
    exe, d = host
    grid = c.grids[compress]
    for k in (1, 8):
        e, _, cnt = run_fixture(c, grid, k, counters=True, records=False)
        we, _, counts = SG.host_walk(exe, d, grid.download(mem), c.tris, c.segments, k, query_labels=c.ql, tri_labels=c.tl)
        NK.assert_lists_equal(e, we, f"{c.name} compress={compress} k={k} against the host walk over the device's grid")
        assert cnt.tolist() == [c.n] + [int(counts[:, j].sum()) for j in range(4)]
        assert cnt[4] == (e["id"][:, k - 1] >= 0).sum() and 0 < cnt[4] < c.n and cnt[2] > 0 and cnt[3] > 0
    # the totals are ADDED: a second launch doubles them
    d_e = mem.alloc(8 * c.n * 8)
    G.assert_totals_added(lambda d_cnt: api.segment_tris(grid, c.d_tris, c.d_segments, c.n, 8, entries=d_e, query_labels=c.d_ql, tri_labels=c.d_tl, counters=d_cnt), mem, cnt)
    mem.free(d_e)


def test_batch_shapes(case):
    """batch sizes 1, 63, 64, 65 and 4095 at odd offsets into the segment buffer"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[True]
    # no segments: nothing is launched, null buffers are fine
    api.segment_tris(grid, c.d_tris, 0, 0, 8)
    api.segment_tris(grid, 0, 0, 0, 1)
    for n, first in ((1, 0), (63, 5), (64, 1671), (65, 4031), (4095, 1)):
        for k in (3, 8):
            e, r = run_segments(api, mem, grid, c.d_tris, c.d_segments + 32 * first, n, k, d_query_labels=c.d_ql + 8 * first, d_tri_labels=c.d_tl)
            NK.assert_lists_equal(e, c.want[first:first + n, :k], f"{c.name} n={n} first={first} k={k}")
            assert (r["id"] == e["id"]).all() and (K.bits(r["d2"]) == K.bits(e["d2"])).all()


CASES = [(name, stage) for name in D.WALKED for stage in D.stages_of(name)]


@pytest.fixture(scope="module")
def deep_mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


def deep_segments(tris):
    """as tests/test_segments_cpu.py: the points of _deep_grids as segments, each to the next one but 17, every fourth of no length, every fourth short"""
    p = D.points(tris)
    s = scene.make_segments(p[:, 0:3], np.roll(p[:, 0:3], 17, axis=0), p[:, 3])
    s[0::4, 4:7] = s[0::4, 0:3]
    s[1::4, 4:7] = s[1::4, 0:3] + (s[1::4, 4:7] - s[1::4, 0:3]) * np.float32(0.01)
    return s


@pytest.mark.parametrize("name,stage", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_deep_grids(deep_mem, host, name, stage):
    """every stage of every catalogue scene, k = 8, against the host brute force"""
    from hagrid_amd import api
    mem = deep_mem
    exe, d = host
    tris = D.make_tris(name)
    s = deep_segments(tris)
    want_e, want_r = SG.host_brute(exe, d, tris, s, 8)
    d_tris = mem.upload(tris); d_s = mem.upload(s)
    dev = D.DeviceStages(name, api, mem, d_tris, tris.shape[0])
    for st in D.STAGES[:D.STAGES.index(stage) + 1]:
        D.stage_grid(dev, st)
    e, r = run_segments(api, mem, dev.grid, d_tris, d_s, s.shape[0], 8)
    NK.assert_lists_equal(e, want_e, f"{name} after {stage}: entries")
    NK.assert_lists_equal(r, want_r, f"{name} after {stage}: records")
    dev.grid.free(); mem.free(d_s); mem.free(d_tris)


def test_live_case(tmp_path):
    """100 000 triangles, 16 384 segments (short ones near the surface, axis-aligned, long diagonals with r = 1 % of the diagonal, ends outside the grid with r = 0.5 %,
    shuffled), k = 8: the device against the host walk over the SAME grid arrays (downloaded), counters included, and against the numpy statement for
    the first 48 segments"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    lo, hi = scene.tris_bbox(tris)
    diag = K.diagonal(lo, hi)
    n = 16384
    s = np.concatenate([scene.make_segments_short(tris, lo, hi, n // 2, 11), scene.make_segments_axis(lo, hi, n // 4, 12),
                        scene.make_segments_diagonal(lo, hi, n // 8, 13, r=np.float32(0.01) * diag),
                        scene.make_segments_outside(lo, hi, n // 8, 14, r=np.float32(0.005) * diag)])
    s = np.ascontiguousarray(s[np.random.default_rng(5).permutation(n)])
    c = G.upload_case(tris); mem, d_tris = c.mem, c.d_tris
    d_s = mem.upload(s)
    exe = SG.build_host(tmp_path)
    for compress in (False, True):
        grid = api.build_all(mem, d_tris, tris.shape[0], compress=compress)
        e, r, cnt = run_segments(api, mem, grid, d_tris, d_s, n, 8, counters=True)
        we, wr, counts = SG.host_walk(exe, tmp_path, grid.download(mem), tris, s, 8)
        NK.assert_lists_equal(e, we, f"soup 100k compress={compress} against the host walk: entries")
        NK.assert_lists_equal(r, wr, f"soup 100k compress={compress} against the host walk: records")
        assert cnt.tolist() == [n] + [int(counts[:, j].sum()) for j in range(4)]
        if not compress:
            se, sr = scene.segment_tris(tris, s[:48], 8)
            NK.assert_lists_equal(e[:48], se, "soup 100k against the statement: entries")
            NK.assert_lists_equal(r[:48], sr, "soup 100k against the statement: records")
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
    d_cur = mem.alloc(8 * n + 64); d_ql = mem.alloc(8 * n + 64); d_tl = mem.alloc(12 * c.tris.shape[0] + 64)
    mem.zero(d_cur, 8 * n + 64); mem.zero(d_ql, 8 * n + 64); mem.zero(d_tl, 12 * c.tris.shape[0] + 64)
    vp = G.vp

    def call(g=grid, tris=c.d_tris, segments=c.d_segments, num=n, k=8, cursors=0, ql=0, tl=0, entries=d_e, records=d_r, counters=0, flags=0):
        return L.hagrid_segment_tris(mem._ctx, G.pod(g), vp(tris), vp(segments), num, k, vp(cursors), vp(ql), vp(tl), vp(entries),
                                     vp(records), vp(counters), flags)

    assert call(counters=d_cnt, cursors=d_cur, ql=d_ql, tl=d_tl) == 0
    assert call(g=None) == EINVAL and call(tris=0) == EINVAL and call(segments=0) == EINVAL and call(num=-1) == EINVAL
    for k in (0, -1, 9, 1 << 20):
        assert call(k=k) == EINVAL
    for flags in (1, 2, 1 << 31):
        assert call(flags=flags) == EINVAL
        assert b"flag" in L.hagrid_last_error(mem._ctx) and b"segment_tris" in L.hagrid_last_error(mem._ctx)
    assert call(entries=0, records=0) == EINVAL
    assert call(entries=0) == 0 and call(records=0) == 0
    assert call(ql=d_ql) == EINVAL and call(tl=d_tl) == EINVAL
    assert call(tris=c.d_tris + 4) == EINVAL and call(segments=c.d_segments + 8, num=n - 1) == EINVAL
    assert call(entries=d_e + 4) == EINVAL and call(records=d_r + 8) == EINVAL and call(cursors=d_cur + 4) == EINVAL
    assert call(ql=d_ql + 2, tl=d_tl) == EINVAL and call(ql=d_ql, tl=d_tl + 2) == EINVAL and call(counters=d_cnt + 4) == EINVAL
    assert call(num=(1 << 31) // 8 + 1, k=8) == ERANGE and call(num=2 ** 31 - 1, k=2) == ERANGE
    assert call(num=0, tris=0, segments=0, entries=0, records=0) == 0
    assert L.hagrid_segment_tris(None, G.pod(grid), vp(c.d_tris), vp(c.d_segments), n, 8, None, None, None, vp(d_e), None, None, 0) == EINVAL
    with pytest.raises(api.HagridError, match="aligned"):
        api.segment_tris(grid, c.d_tris, c.d_segments + 4, 8, 8, entries=d_e)
    # a grid given up for traversal has no construction format left; a bad shift
    g2 = api.build_all(mem, c.d_tris, c.tris.shape[0])
    shift = g2.pod.shift
    g2.pod.shift = 16
    assert call(g=g2) == EINVAL and b"shift" in L.hagrid_last_error(mem._ctx)
    g2.pod.shift = shift
    with G.released_grid(c, g2) as released:
        if released is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.segment_tris(g2, c.d_tris, c.d_segments, n, 8, entries=d_e)
            assert call(g=g2, num=0) == EINVAL
    for p in (d_e, d_r, d_cnt, d_cur, d_ql, d_tl):
        mem.free(p)
    api.setup_traversal(grid)
    e, _ = run_fixture(c, grid, 8, records=False)
    NK.assert_lists_equal(e, c.want, f"{c.name} after the refused calls")
