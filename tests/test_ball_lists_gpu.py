"""Ball lists on the GPU (ball_refs_kernel and unique_lists_kernel of hagrid_amd/csrc/ball_lists.hip): the protocol count -> scan -> fill -> unique -> scan ->
compact on Cell and SmallCell grids built on the device, into poisoned and guarded buffers, against the fixture tests/golden/ball_lists.npz and the host brute
force; the filled references BEFORE the sort and the six counters against the host walk over the downloaded grid; a traversal image present, ray binning on,
no image, the nearest-hit path unmoved; too little room and a clipped capacity; the second stage alone on the synthetic segments; batch shapes; the deep
grids at every stage; a live case; api.ball_lists on a torch stream against api.tris_within; every argument error; the kernel budget.
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import numpy as np
import pytest

import _ball_lists as BL
import _closest as K
import _deep_grids as D
import _gpu_case as G
import _nearest_k as NK
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

EINVAL = G.EINVAL
ENTRY = BL.ENTRY


@pytest.fixture(scope="module")
def fixture():
    return np.load(BL.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("ball_lists_host_gpu")
    return BL.build_host(d), d


@pytest.fixture(scope="module", params=K.SCENES)
def case(request, fixture, host):
    """one scene of the fixture: Cell and SmallCell grids built on the device, the queries uploaded, the host brute force made once"""
    c = G.open_case(request.param, K.make_tris(request.param))
    c.queries = BL.queries(c.tris)
    c.n = c.queries.shape[0]
    c.d_points = c.mem.upload(c.queries)
    exe, d = host
    c.want = BL.host_brute(exe, d, c.tris, c.queries)
    for v in c.want.values():
        v.setflags(write=False)
    assert (np.diff(c.want["offsets"]) == fixture[c.name + "_sizes"]).all()
    BL.assert_csr_equal(BL.csr_slice(c.want, BL.STORED), BL.fixture_csr(fixture, c.name), f"{c.name}: the brute force against the fixture")
    c.walks = {}
    yield c
    c.mem.close()


def host_walk(c, host, compress):
    """the protocol on the host over the device's grid (downloaded): once per grid"""
    if compress not in c.walks:
        exe, d = host
        c.walks[compress] = BL.host_lists(exe, d, c.grids[compress].download(c.mem), c.tris, c.queries)
        BL.assert_csr_equal(c.walks[compress], c.want, f"{c.name}: the host walk over the device's grid against the brute force")
    return c.walks[compress]


def check_device(c, host, compress, what):
    got = BL.device_lists(c, c.grids[compress], c.d_points, c.n)
    BL.assert_csr_equal(got, c.want, f"{c.name} compress={compress} {what}")
    return got


@pytest.mark.parametrize("compress", [False, True])
def test_device_lists_equal_fixture_and_brute_force(case, host, fixture, compress):
    """all 4096 lists against the brute force (which the fixture pins), with the image present, with ray binning set, and with traverse.image = 0; the filled
    references before the sort are the host walk's, in order; the six counters are the host walk's; the stages' own counters"""
    c = case; mem = c.mem
    grid = c.grids[compress]
    with G.image_present(c, grid):
        got = check_device(c, host, compress, "image present")
        mem.set_ray_binning(1)
        check_device(c, host, compress, "binning set")
    G.drop_image(c, grid)
    check_device(c, host, compress, "traverse.image=0")
    mem.set_option("traverse.image", 2)
    BL.assert_csr_equal(BL.csr_slice(got, BL.STORED), BL.fixture_csr(fixture, c.name), f"{c.name}: the device against the fixture")
    w = host_walk(c, host, compress)
    assert (got["refs"] == w["refs"]).all(), "R per query"
    assert (BL.words(got["ref_entries"]) == BL.words(w["ref_entries"])).all(), "the references before the sort, in walk order"
    assert got["totals"].tolist() == w["totals"].tolist(), (got["totals"], w["totals"])
    m = np.diff(c.want["offsets"])
    assert got["unique_totals"].tolist() == [c.n, int(got["refs"].sum()), int(m.sum()), int((got["refs"] > BL.SORT_CAP).sum())]
    assert got["compact_totals"].tolist() == [c.n, int(m.sum()), 0, 0]
    assert (got["refs"] > BL.SORT_CAP).sum() >= 8 and ((got["refs"] > 64) & (got["refs"] <= BL.SORT_CAP)).sum() > 100 and (got["refs"] <= 1).sum() > 100
    # after unique: survivors at the front, EMPTY behind them
    ro = got["ref_offsets"]
    tail = np.concatenate([np.arange(ro[i] + m[i], ro[i + 1]) for i in range(c.n)])
    assert (BL.words(got["sorted_entries"])[tail] == BL.words(scene.empty_entry())).all()


def test_counters_are_added_and_nearest_hit_unmoved(case, host):
    """the fill launch on counters that hold its own totals doubles them; a nearest-hit launch before and after the protocol gives the same hits, the hints kept for
    the ray buffer unchanged"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    mem.set_option("traverse.image", 2)
    api.setup_traversal(grid)
    with G.nearest_hit_unmoved(c, grid):
        got = check_device(c, host, False, "between two nearest-hit launches")
    d_ro = mem.upload(got["ref_offsets"])
    total = int(got["ref_offsets"][-1])
    d_e = mem.alloc(8 * total)
    G.assert_totals_added(lambda d_tot: api.ball_refs(grid, c.d_tris, c.d_points, c.n, offsets=d_ro, entries=d_e, capacity=total, counters=d_tot), mem, got["totals"])
    d_m = mem.alloc(4 * c.n)
    G.assert_totals_added(lambda d_tot: api.unique_lists(c.n, d_ro, d_e, total, d_m, counters=d_tot, mem=mem), mem,
                          np.array([c.n, total, int(c.want["offsets"][-1]), int((got["refs"] > BL.SORT_CAP).sum())], np.int64))
    for p in (d_ro, d_e, d_m):
        mem.free(p)


def test_too_little_room_and_clipped_capacity(case, host):
    """fill mode with rooms that are too small, too large, and ranges the capacity cuts off: a prefix of the walk's references, the EMPTY entry in what is left,
    the overflow counted, nothing outside the ranges -- slot for slot what the host walk leaves in the same poisoned buffer"""
    c = case; api, mem = c.api, c.mem
    exe, d = host
    w = host_walk(c, host, True)
    refs = w["refs"].astype(np.int64)
    rng = np.random.RandomState(3)
    room = refs.copy()
    how = rng.randint(0, 4, size=c.n)
    room[how == 0] = refs[how == 0] // 2
    room[how == 1] += 5
    off = np.zeros(c.n + 1, np.int64); np.cumsum(room, out=off[1:])
    off += 3                                            # three slots in front belong to nobody
    capacity = int(off[c.n - 40])                       # the last 40 ranges leave the capacity: room 0
    arrays = c.grids[True].download(mem)
    counts, totals, want = BL.host_refs(exe, d, arrays, c.tris, c.queries, offsets=off, entries=BL.poisoned(capacity))
    d_off = mem.upload(off)
    d_e = P.alloc_out(mem, 8 * capacity)
    d_cnt = P.alloc_out(mem, 4 * c.n)
    d_tot = mem.alloc(48); mem.zero(d_tot, 48)
    api.ball_refs(c.grids[True], c.d_tris, c.d_points, c.n, counts=d_cnt, offsets=d_off, entries=d_e, capacity=capacity, counters=d_tot)
    mem.synchronize()
    got = P.fetch(mem, d_e, ENTRY, capacity)
    assert (BL.words(got) == BL.words(want)).all()
    assert (BL.words(got)[:3] == BL.POISON).all()
    assert (P.fetch(mem, d_cnt, np.int32, c.n) == refs).all(), "R does not depend on the room"
    t = mem.download(d_tot, np.int64, 6)
    assert t.tolist() == totals.tolist() and t[5] > 40 and 0 < t[4] < refs.sum()
    for p in (d_off, d_e, d_cnt, d_tot):
        mem.free(p)


def test_unique_and_compact_alone(case):
    """the second stage on the synthetic segments of the CPU suite (every length at which the kernel takes another path; duplicates, EMPTY, NaN, +-0.0, refused
    ranges): every word of the buffer is scene.unique_lists', the counts too; compact into too little room is scene.compact_lists'"""
    c = case; api, mem = c.api, c.mem
    offsets, entries, capacity = BL.synthetic_segments()
    n = offsets.size - 1
    want_e, want_c = scene.unique_lists(offsets, entries)
    d_off = mem.upload(offsets)
    d_e = mem.upload(np.concatenate([np.ascontiguousarray(entries).view(np.uint8), np.full(P.GUARD, 0xFF, np.uint8)]))        # the segments and a guard behind them
    d_cnt = P.alloc_out(mem, 4 * n)
    d_tot = mem.alloc(32); mem.zero(d_tot, 32)
    target = d_e
    api.unique_lists(n, d_off, target, capacity, d_cnt, counters=d_tot, mem=mem)
    mem.synchronize()
    got_e = P.fetch(mem, d_e, ENTRY, capacity).copy()
    got_c = P.fetch(mem, d_cnt, np.int32, n).copy()
    assert (got_c == want_c).all(), np.flatnonzero(got_c != want_c)[:5]
    bad = np.flatnonzero(BL.words(got_e) != BL.words(want_e))
    assert bad.size == 0, f"{bad.size} slots differ, the first at {bad[:5]}"
    room = scene._segment_ranges(offsets, capacity)[1]
    assert mem.download(d_tot, np.int64, 4).tolist() == [n, int(room.sum()), int(want_c.sum()), int((room > BL.SORT_CAP).sum())]
    out_offsets, out_capacity = BL.tight_destination(want_c)
    want_o = scene.compact_lists(offsets, want_e, want_c, out_offsets, out_capacity, fill=BL.poisoned(out_capacity))
    d_oo = mem.upload(out_offsets)
    d_out = P.alloc_out(mem, 8 * out_capacity)
    mem.zero(d_tot, 32)
    api.compact_lists(n, d_off, target, capacity, d_cnt, d_oo, d_out, out_capacity, counters=d_tot, mem=mem)
    mem.synchronize()
    got_o = P.fetch(mem, d_out, ENTRY, out_capacity)
    assert (BL.words(got_o) == BL.words(want_o)).all()
    droom = scene._segment_ranges(out_offsets, out_capacity)[1]
    copied = np.minimum(np.minimum(want_c, room), droom)
    assert mem.download(d_tot, np.int64, 4).tolist() == [n, int(copied.sum()), int((want_c > copied).sum()), 0]
    for p in (d_off, d_e, d_cnt, d_tot, d_oo, d_out):
        mem.free(p)


def test_batch_shapes(case):
    """batches of 1, 63, 65 and 4095 queries starting at offsets into the query buffer"""
    c = case
    for n, first in ((1, 2048), (63, 5), (65, 4031), (4095, 1)):
        got = BL.device_lists(c, c.grids[True], c.d_points + 16 * first, n)
        BL.assert_csr_equal(got, BL.csr_slice(c.want, np.arange(first, first + n)), f"{c.name} n={n} first={first}")


def test_labels_on_the_device(host):
    """_nearest_k.stadium_labels on the device against scene.tris_within with the labels"""
    tris, F, q, labels = NK.stadium_labels()
    c = G.upload_case(tris)
    grid = c.api.build_all(c.mem, c.d_tris, tris.shape[0], compress=True)
    d_q, d_ql, d_tl = c.mem.upload(q), c.mem.upload(labels), c.mem.upload(F)
    got = BL.device_lists(c, grid, d_q, q.shape[0], d_query_labels=d_ql, d_tri_labels=d_tl)
    BL.assert_csr_equal(got, scene.tris_within(tris, q, query_labels=labels, tri_labels=F), "labelled lists against the statement")
    c.mem.close()


CASES = [(name, stage) for name in D.WALKED for stage in D.stages_of(name)]


@pytest.fixture(scope="module")
def deep_mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


def deep_points(tris):
    """_deep_grids.points with every r = inf replaced by 20 % of the diagonal (as the CPU suite)"""
    pts = D.points(tris)
    lo, hi = scene.tris_bbox(tris)
    pts[np.isposinf(pts[:, 3]), 3] = np.float32(0.2) * scene.bbox_diagonal(lo, hi)
    return pts


@pytest.mark.parametrize("name,stage", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_deep_grids(deep_mem, host, name, stage):
    """every stage of every catalogue scene against the host brute force"""
    from hagrid_amd import api
    mem = deep_mem
    exe, d = host
    tris = D.make_tris(name)
    pts = deep_points(tris)
    want = BL.host_brute(exe, d, tris, pts)
    c = G.Case(); c.api, c.mem, c.tris = api, mem, tris
    c.d_tris = mem.upload(tris); d_pts = mem.upload(pts)
    dev = D.DeviceStages(name, api, mem, c.d_tris, tris.shape[0])
    for st in D.STAGES[:D.STAGES.index(stage) + 1]:
        D.stage_grid(dev, st)
    BL.assert_csr_equal(BL.device_lists(c, dev.grid, d_pts, pts.shape[0]), want, f"{name} after {stage}")
    dev.grid.free(); mem.free(d_pts); mem.free(c.d_tris)


def test_live_case(tmp_path):
    """100 000 triangles, 8 192 queries (near the surface and uniform, r = 2 % of the diagonal, shuffled): the device against the host walk over the SAME grid
    arrays (downloaded) -- references in order, counters, lists -- and against the numpy statement for the first 128 queries"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    lo, hi = scene.tris_bbox(tris)
    n = 8192
    q = np.empty((n, 4), dtype=np.float32); q[:, 3] = np.float32(0.02) * K.diagonal(lo, hi)
    q[:n // 2, 0:3] = K.near_surface_points(tris, lo, hi, n // 2, 11)
    q[n // 2:, 0:3] = K.uniform_points(lo, hi, n // 2, 12)
    q = np.ascontiguousarray(q[np.random.default_rng(5).permutation(n)])
    c = G.upload_case(tris); mem = c.mem
    d_pts = mem.upload(q)
    exe = BL.build_host(tmp_path)
    for compress in (False, True):
        grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=compress)
        got = BL.device_lists(c, grid, d_pts, n)
        w = BL.host_lists(exe, tmp_path, grid.download(mem), tris, q)
        BL.assert_csr_equal(got, w, f"soup 100k compress={compress} against the host walk")
        assert (BL.words(got["ref_entries"]) == BL.words(w["ref_entries"])).all() and got["totals"].tolist() == w["totals"].tolist()
        if not compress:
            BL.assert_csr_equal(BL.csr_slice(got, np.arange(128)), scene.tris_within(tris, q[:128]), "soup 100k against the statement")
            assert np.median(np.diff(got["offsets"])) > 8
        grid.free()
    mem.close()


def test_ball_lists_on_a_torch_stream(case):
    """api.ball_lists with torch tensors on a torch stream equals api.tris_within key for key (RADIUS and the first 64 NEAR queries), and the brute force"""
    import torch
    c = case; api, mem = c.api, c.mem
    which = np.concatenate([np.arange(K.RADIUS.start, K.RADIUS.stop), np.arange(64)])
    qs = np.ascontiguousarray(c.queries[which])
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_pts = torch.from_numpy(qs).cuda()
            got = api.ball_lists(c.grids[True], c.d_tris, t_pts)
            paged = api.tris_within(c.grids[True], c.d_tris, t_pts)
            stream.synchronize()
            assert paged["complete"]
            for key in ("offsets", "ids", "d2"):
                assert got[key].dtype == paged[key].dtype and got[key].shape == paged[key].shape, key
                assert (got[key].cpu().numpy().view(np.uint32 if key == "d2" else got[key].cpu().numpy().dtype) ==
                        paged[key].cpu().numpy().view(np.uint32 if key == "d2" else paged[key].cpu().numpy().dtype)).all(), key
            BL.assert_csr_equal({k: got[k].cpu().numpy() for k in ("offsets", "ids", "d2")}, BL.csr_slice(c.want, which), f"{c.name}: api.ball_lists against the brute force")
            assert got["refs"] >= int(got["offsets"][-1].item()) > qs.shape[0]
            empty = api.ball_lists(c.grids[True], c.d_tris, t_pts[:0])
            assert empty["offsets"].tolist() == [0] and empty["ids"].numel() == 0 and empty["refs"] == 0
    finally:
        mem.use_stream(None)


def test_errors_leave_the_context_working(case, host):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    n = c.n
    vp = G.vp
    cap = 1 << 16
    d_e = mem.alloc(8 * cap + 64); d_cnt = mem.alloc(4 * n + 64); d_tot = mem.alloc(64); d_off = mem.alloc(8 * (n + 1) + 64)
    d_ql = mem.alloc(4 * n + 64); d_tl = mem.alloc(12 * c.tris.shape[0] + 64)
    mem.zero(d_off, 8 * (n + 1) + 64); mem.zero(d_ql, 4 * n + 64); mem.zero(d_tl, 12 * c.tris.shape[0] + 64); mem.zero(d_tot, 64)

    def refs(g=grid, tris=c.d_tris, points=c.d_points, num=n, ql=0, tl=0, offsets=d_off, counts=d_cnt, entries=d_e, capacity=cap, counters=0, flags=0):
        return L.hagrid_ball_refs(mem._ctx, G.pod(g), vp(tris), vp(points), num, vp(ql), vp(tl), vp(offsets), vp(counts), vp(entries), capacity, vp(counters), flags)

    assert refs(counters=d_tot, ql=d_ql, tl=d_tl) == 0                        # (every room is 0: the offsets are zeros)
    assert refs(offsets=0, entries=0, capacity=0) == 0                        # count mode
    assert refs(g=None) == EINVAL and refs(tris=0) == EINVAL and refs(points=0) == EINVAL and refs(num=-1) == EINVAL and refs(capacity=-1) == EINVAL
    for flags in (1, 2, 1 << 31):
        assert refs(flags=flags) == EINVAL and b"flag" in L.hagrid_last_error(mem._ctx)
    assert refs(offsets=0) == EINVAL and refs(offsets=0, entries=0) == EINVAL and refs(offsets=0, entries=0, capacity=0, counts=0) == EINVAL
    assert refs(entries=0) == EINVAL and refs(entries=0, capacity=0) == 0 and refs(counts=0) == 0
    assert refs(ql=d_ql) == EINVAL and refs(tl=d_tl) == EINVAL
    assert refs(tris=c.d_tris + 4) == EINVAL and refs(points=c.d_points + 8, num=n - 1) == EINVAL
    assert refs(entries=d_e + 4) == EINVAL and refs(offsets=d_off + 4) == EINVAL and refs(counts=d_cnt + 2) == EINVAL and refs(counters=d_tot + 4) == EINVAL
    assert refs(ql=d_ql + 2, tl=d_tl) == EINVAL and refs(ql=d_ql, tl=d_tl + 2) == EINVAL
    assert refs(num=0, tris=0, points=0, offsets=0, counts=0, entries=0, capacity=0) == 0
    assert L.hagrid_ball_refs(None, G.pod(grid), vp(c.d_tris), vp(c.d_points), n, None, None, None, vp(d_cnt), None, 0, None, 0) == EINVAL

    def uniq(num=n, offsets=d_off, entries=d_e, capacity=cap, counts=d_cnt, counters=0, flags=0):
        return L.hagrid_unique_lists(mem._ctx, num, vp(offsets), vp(entries), capacity, vp(counts), vp(counters), flags)

    def comp(num=n, offsets=d_off, entries=d_e, capacity=cap, counts=d_cnt, out_offsets=d_off, out_entries=d_e, out_capacity=cap, counters=0, flags=0):
        return L.hagrid_compact_lists(mem._ctx, num, vp(offsets), vp(entries), capacity, vp(counts), vp(out_offsets), vp(out_entries), out_capacity, vp(counters), flags)

    for f in (uniq, comp):
        assert f(counters=d_tot) == 0
        assert f(num=-1) == EINVAL and f(capacity=-1) == EINVAL and f(flags=1) == EINVAL and f(offsets=0) == EINVAL and f(counts=0) == EINVAL and f(entries=0) == EINVAL
        assert f(offsets=d_off + 4) == EINVAL and f(entries=d_e + 4) == EINVAL and f(counts=d_cnt + 2) == EINVAL and f(counters=d_tot + 4) == EINVAL
        assert f(entries=0, capacity=0) == 0 and f(num=0, offsets=0, counts=0, entries=0) == 0
    assert comp(out_capacity=-1) == EINVAL and comp(out_offsets=0) == EINVAL and comp(out_entries=0) == EINVAL and comp(out_entries=d_e + 4) == EINVAL
    assert comp(out_offsets=d_off + 4) == EINVAL and comp(out_entries=0, out_capacity=0) == 0
    assert L.hagrid_unique_lists(None, n, vp(d_off), vp(d_e), cap, vp(d_cnt), None, 0) == EINVAL
    assert L.hagrid_compact_lists(None, n, vp(d_off), vp(d_e), cap, vp(d_cnt), vp(d_off), vp(d_e), cap, None, 0) == EINVAL
    with pytest.raises(api.HagridError, match="aligned"):
        api.ball_refs(grid, c.d_tris, c.d_points + 4, 8, counts=d_cnt)
    # a grid given up for traversal has no construction format left; a bad shift
    g2 = api.build_all(mem, c.d_tris, c.tris.shape[0])
    shift = g2.pod.shift
    g2.pod.shift = 16
    assert refs(g=g2) == EINVAL and b"shift" in L.hagrid_last_error(mem._ctx)
    g2.pod.shift = shift
    with G.released_grid(c, g2) as released:
        if released is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.ball_refs(g2, c.d_tris, c.d_points, n, counts=d_cnt)
            assert refs(g=g2, num=0) == EINVAL
    mem.synchronize()
    for p in (d_e, d_cnt, d_tot, d_off, d_ql, d_tl):
        mem.free(p)
    api.setup_traversal(grid)
    which = np.arange(K.RADIUS.start, K.RADIUS.stop)
    BL.assert_csr_equal(BL.device_lists(c, grid, c.d_points + 16 * K.RADIUS.start, which.size), BL.csr_slice(c.want, which), f"{c.name} after the refused calls")


def test_kernel_budget():
    G.kernel_budget(G.kernel_listing(), one_each=("ball_refs_kernel", "unique_lists_kernel"))
