"""Overlap lists on the GPU (overlap_refs_kernel of hagrid_amd/csrc/overlap_lists.hip, then unique_lists_kernel): the protocol count -> scan -> fill -> unique ->
scan -> compact for boxes, contact queries and oriented boxes on Cell and SmallCell grids built on the device, into poisoned and guarded buffers, against the
fixtures of the k-list queries and the host brute force; the filled references BEFORE the sort and the six counters against the host walk over the downloaded
grid; a traversal image present (all 4096 queries), ray binning on and no image (256 of them: queries 2048 .. 2303), the nearest-hit path unmoved; too little room and a clipped capacity; batch shapes; the deep grids
at every stage; api.box_lists, api.contact_lists and api.obb_lists on a torch stream against the paged forms; every argument error; the kernel budget.
The case and what every query's file checks around its own launches come from tests/_gpu_case.py.  Every comparison is equality."""
import numpy as np
import pytest

import _deep_grids as D
import _gpu_case as G
import _obb as OB
import _overlap_lists as OL
import _overlap_tris as W
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

EINVAL = G.EINVAL
ENTRY = OL.ENTRY


@pytest.fixture(scope="module")
def fixtures():
    return {shape: np.load(path) for shape, path in OL.FIXTURES.items()}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_lists_host_gpu")
    return OL.build_host(d), d


@pytest.fixture(scope="module", params=OL.SCENES)
def case(request, fixtures, host):
    """one scene of the fixtures: Cell and SmallCell grids built on the device, the queries of the three shapes uploaded, the host brute forces made once
    and pinned to the fixtures"""
    c = G.open_case(request.param, OL.make_tris(request.param))
    exe, d = host
    c.batch, c.dev, c.want, c.walks = {}, {}, {}, {}
    for shape in OL.SHAPES:
        b = OL.fixture_batch(shape, fixtures[shape], c.name, c.tris)
        c.batch[shape] = b
        c.dev[shape] = OL.DeviceBatch(c.mem, b)
        c.want[shape] = OL.host_brute(exe, d, c.tris, b, grid=(c.grids[False].bbox_min, c.grids[False].bbox_max))
        for v in c.want[shape].values():
            v.setflags(write=False)
        OL.assert_fixture(c.want[shape], fixtures[shape], c.name, f"{shape} {c.name}: the brute force against the fixture")
    yield c
    c.mem.close()


def host_walk(c, host, shape, compress):
    """the protocol on the host over the device's grid (downloaded): once per shape and grid"""
    key = (shape, compress)
    if key not in c.walks:
        exe, d = host
        c.walks[key] = OL.host_lists(exe, d, c.grids[compress].download(c.mem), c.tris, c.batch[shape])
        OL.assert_csr_equal(c.walks[key], c.want[shape], f"{shape} {c.name}: the host walk over the device's grid against the brute force")
    return c.walks[key]


def check_device(c, shape, compress, what):
    got = OL.device_lists(c, c.grids[compress], c.dev[shape])
    OL.assert_csr_equal(got, c.want[shape], f"{shape} {c.name} compress={compress} {what}")
    return got


def check_part(c, shape, compress, what, n=256, skip=2048):
    """the same for n queries from query `skip` on: what the settings that must not matter are tried with"""
    got = OL.device_lists(c, c.grids[compress], c.dev[shape], n, skip)
    OL.assert_csr_equal(got, OL.csr_slice(c.want[shape], np.arange(skip, skip + n)), f"{shape} {c.name} compress={compress} {what}")


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("shape", OL.SHAPES)
def test_device_lists_equal_fixture_and_brute_force(case, host, fixtures, shape, compress):
    """all 4096 lists against the brute force and the fixture with the image present; 256 of them again with ray binning set and with traverse.image = 0; the filled references
    before the sort are the host walk's, in order; the six counters are the host walk's; the stages' own counters; the sort paths reached"""
    c = case; mem = c.mem
    grid = c.grids[compress]
    with G.image_present(c, grid):
        got = check_device(c, shape, compress, "image present")
        mem.set_ray_binning(1)
        check_part(c, shape, compress, "binning set")
    G.drop_image(c, grid)
    check_part(c, shape, compress, "traverse.image=0")
    mem.set_option("traverse.image", 2)
    OL.assert_fixture(got, fixtures[shape], c.name, f"{shape} {c.name}: the device against the fixture")
    w = host_walk(c, host, shape, compress)
    assert (got["refs"] == w["refs"]).all(), "R per query"
    assert (OL.words(got["ref_entries"]) == OL.words(w["ref_entries"])).all(), "the references before the sort, in walk order"
    assert got["totals"].tolist() == w["totals"].tolist(), (got["totals"], w["totals"])
    m = np.diff(c.want[shape]["offsets"]); R = got["refs"]; n = c.batch[shape].n
    assert got["totals"][4] == R.sum() and got["totals"][5] == 0
    assert got["unique_totals"].tolist() == [n, int(R.sum()), int(m.sum()), int((R > OL.SORT_CAP).sum())]
    assert got["compact_totals"].tolist() == [n, int(m.sum()), 0, 0]
    if shape == "contact":
        assert (R >= 2).sum() >= 100
    else:
        assert (R > OL.SORT_CAP).sum() >= 8 and ((R > 64) & (R <= OL.SORT_CAP)).sum() > 100
    assert (R <= 1).sum() > 100
    # after unique: survivors at the front, EMPTY behind them
    ro = got["ref_offsets"]
    tail = np.concatenate([np.arange(ro[i] + m[i], ro[i + 1]) for i in range(n)])
    assert (OL.words(got["sorted_entries"])[tail] == OL.words(scene.empty_entry())).all()


@pytest.mark.parametrize("shape", OL.SHAPES)
def test_counters_are_added_and_nearest_hit_unmoved(case, shape):
    """the fill launch on counters that hold its own totals doubles them; a nearest-hit launch before and after the protocol gives the same hits, the hints
    kept for the ray buffer unchanged"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    mem.set_option("traverse.image", 2)
    api.setup_traversal(grid)
    with G.nearest_hit_unmoved(c, grid):
        got = check_device(c, shape, False, "between two nearest-hit launches")
    d_ro = mem.upload(got["ref_offsets"])
    total = int(got["ref_offsets"][-1])
    d_e = mem.alloc(8 * total)
    G.assert_totals_added(lambda d_tot: OL.device_refs(api, grid, c.d_tris, c.dev[shape], offsets=d_ro, entries=d_e, capacity=total, counters=d_tot), mem, got["totals"])
    mem.free(d_ro); mem.free(d_e)


@pytest.mark.parametrize("shape", OL.SHAPES)
def test_too_little_room_and_clipped_capacity(case, host, shape):
    """fill mode with rooms that are too small, too large, three unowned slots in front and the last 40 ranges beyond the capacity: a prefix of the walk's
    references, the EMPTY entry in what is left, the overflow counted, nothing outside the ranges -- slot for slot what the host walk leaves in the same
    poisoned buffer; counts do not depend on the room"""
    c = case; api, mem = c.api, c.mem
    exe, d = host
    b = c.batch[shape]
    refs = host_walk(c, host, shape, True)["refs"].astype(np.int64)
    rng = np.random.RandomState(3)
    room = refs.copy()
    how = rng.randint(0, 4, size=b.n)
    room[how == 0] = refs[how == 0] // 2
    room[how == 1] += 5
    off = np.zeros(b.n + 1, np.int64); np.cumsum(room, out=off[1:])
    off += 3                                            # three slots in front belong to nobody
    capacity = int(off[b.n - 40])                       # the last 40 ranges leave the capacity: room 0
    counts, totals, want = OL.host_fill(exe, d, c.grids[True].download(mem), c.tris, b, off, OL.poisoned(capacity))
    assert (counts[:, 0] == refs).all()
    d_off = mem.upload(off)
    d_e = P.alloc_out(mem, 8 * capacity)
    d_cnt = P.alloc_out(mem, 4 * b.n)
    d_tot = mem.alloc(48); mem.zero(d_tot, 48)
    OL.device_refs(api, c.grids[True], c.d_tris, c.dev[shape], counts=d_cnt, offsets=d_off, entries=d_e, capacity=capacity, counters=d_tot)
    mem.synchronize()
    got = P.fetch(mem, d_e, ENTRY, capacity)
    assert (OL.words(got) == OL.words(want)).all()
    assert (OL.words(got)[:3] == OL.POISON).all()
    assert (P.fetch(mem, d_cnt, np.int32, b.n) == refs).all(), "R does not depend on the room"
    t = mem.download(d_tot, np.int64, 6)
    assert t.tolist() == totals.tolist() and t[5] > 0 and 0 < t[4] < refs.sum()
    for p in (d_off, d_e, d_cnt, d_tot):
        mem.free(p)


@pytest.mark.parametrize("shape", OL.SHAPES)
def test_batch_shapes(case, shape):
    """batches of 1, 63, 65 and 4095 queries starting at offsets into the query buffer"""
    c = case
    for n, first in ((1, 2048), (63, 5), (65, 4031), (4095, 1)):
        got = OL.device_lists(c, c.grids[True], c.dev[shape], n, first)
        OL.assert_csr_equal(got, OL.csr_slice(c.want[shape], np.arange(first, first + n)), f"{shape} {c.name} n={n} first={first}")


@pytest.mark.parametrize("shape", ["contact", "obb"])
def test_labels_on_the_device(case, fixtures, host, shape):
    """the labelled queries of the fixtures on the device against the fixture's labelled answers and the host brute force"""
    c = case
    exe, d = host
    b = OL.fixture_batch(shape, fixtures[shape], c.name, c.tris, labelled=True)
    db = OL.DeviceBatch(c.mem, b)
    got = OL.device_lists(c, c.grids[True], db)
    OL.assert_fixture(got, fixtures[shape], c.name + "_lab", f"{shape} {c.name}: the labelled device lists")
    OL.assert_csr_equal(got, OL.host_brute(exe, d, c.tris, b, grid=(c.grids[True].bbox_min, c.grids[True].bbox_max)), f"{shape} {c.name}: labelled, against the brute force")
    db.free()


CASES = [(name, stage) for name in D.WALKED for stage in D.stages_of(name)]


@pytest.fixture(scope="module")
def deep_mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


@pytest.mark.parametrize("name,stage", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_deep_grids(deep_mem, host, name, stage):
    """every stage of every catalogue scene, the three shapes, against the host brute force"""
    from hagrid_amd import api
    mem = deep_mem
    exe, d = host
    tris = D.make_tris(name)
    c = G.Case(); c.api, c.mem, c.tris = api, mem, tris
    c.d_tris = mem.upload(tris)
    dev = D.DeviceStages(name, api, mem, c.d_tris, tris.shape[0])
    for st in D.STAGES[:D.STAGES.index(stage) + 1]:
        D.stage_grid(dev, st)
    for b in OL.deep_batches(name, tris):
        want = OL.host_brute(exe, d, tris, b, grid=(dev.grid.bbox_min, dev.grid.bbox_max))
        db = OL.DeviceBatch(mem, b)
        OL.assert_csr_equal(OL.device_lists(c, dev.grid, db), want, f"{name} {b.shape} after {stage}")
        db.free()
    dev.grid.free(); mem.free(c.d_tris)


def test_lists_on_a_torch_stream(case):
    """api.box_lists, api.contact_lists and api.obb_lists with torch tensors on a torch stream: the brute force's lists; obb_lists == api.tris_in_obbs key for key
    (a sub-batch of BIG and PLANK queries, complete); the contact form with first = i + 1 and the scene's labels reproduces every row of
    api.self_intersections as a prefix; empty batches"""
    import torch
    c = case; api, mem = c.api, c.mem
    grid = c.grids[True]
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            which = np.concatenate([np.arange(OB.BIG.start, OB.BIG.start + 24), np.arange(OB.PLANK.start, OB.PLANK.start + 24)])
            t_obbs = torch.from_numpy(np.ascontiguousarray(c.batch["obb"].rows()[which])).cuda()
            got = api.obb_lists(grid, c.d_tris, t_obbs)
            paged = api.tris_in_obbs(grid, c.d_tris, t_obbs)
            stream.synchronize()
            assert paged["complete"] and paged["pages"] > 2
            for key in ("offsets", "ids"):
                assert got[key].dtype == paged[key].dtype and got[key].shape == paged[key].shape, key
                assert (got[key] == paged[key]).all().item(), key
            OL.assert_csr_equal({k: got[k].cpu().numpy() for k in ("offsets", "ids")}, OL.csr_slice(c.want["obb"], which), f"{c.name}: api.obb_lists against the brute force")
            assert got["refs"] >= int(got["offsets"][-1].item()) > which.size

            which = np.concatenate([np.arange(0, 64), np.arange(2048, 2112), np.arange(3840, 3904)])
            t_boxes = torch.from_numpy(np.ascontiguousarray(c.batch["box"].rows()[which])).cuda()
            got = api.box_lists(grid, c.d_tris, t_boxes)
            OL.assert_csr_equal({k: got[k].cpu().numpy() for k in ("offsets", "ids")}, OL.csr_slice(c.want["box"], which), f"{c.name}: api.box_lists against the brute force")

            b = c.batch["contact"]
            which = np.concatenate([np.arange(W.OWN.start, W.OWN.start + 64), np.arange(W.MOVED.start, W.MOVED.start + 64), np.arange(W.PAGED.start, W.PAGED.stop)])
            got = api.contact_lists(grid, c.d_tris, torch.from_numpy(np.ascontiguousarray(b.records[which])).cuda(), first=torch.from_numpy(np.ascontiguousarray(b.first[which])).cuda())
            OL.assert_csr_equal({k: got[k].cpu().numpy() for k in ("offsets", "ids")}, OL.csr_slice(c.want["contact"], which), f"{c.name}: api.contact_lists against the brute force")

            # all self-intersections, each pair once: every row of api.self_intersections is a prefix
            nt = c.tris.shape[0]
            t_tris = torch.from_numpy(c.tris).cuda()
            labels = torch.from_numpy(W.scene_labels(c.name, nt)).cuda()
            g2 = api.build_all(mem, t_tris.data_ptr(), nt, compress=True)
            ids, counts = api.self_intersections(g2, t_tris, labels, 8)
            full = api.contact_lists(g2, t_tris, t_tris, first=torch.arange(1, nt + 1, dtype=torch.int32, device="cuda"), query_labels=labels, tri_labels=labels)
            stream.synchronize()
            off = full["offsets"].cpu().numpy(); fid = full["ids"].cpu().numpy()
            sizes = np.diff(off)
            assert (np.minimum(sizes, 9) == counts.cpu().numpy()).all()
            assert (OL.first_ids({"offsets": off, "ids": fid}) == ids.cpu().numpy()).all()
            assert (fid > np.repeat(np.arange(nt), sizes)).all(), "each pair once, at its smaller id"
            if c.name == "soup":
                assert sizes.sum() > 100
            g2.free()

            for empty in (api.obb_lists(grid, c.d_tris, t_obbs[:0]), api.box_lists(grid, c.d_tris, t_boxes[:0]), api.contact_lists(grid, c.d_tris, t_tris[:0])):
                assert empty["offsets"].tolist() == [0] and empty["ids"].numel() == 0 and empty["refs"] == 0
            stream.synchronize()
    finally:
        mem.use_stream(None)


def test_errors_leave_the_context_working(case):
    """every refusal of the three entry points: those of the k-list query of the same shape (a released grid, a bad shift, misaligned buffers, labels given
    singly) and those of hagrid_ball_refs (fill mode without offsets or entries, a negative capacity, any flag); a correct launch afterwards"""
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    vp = G.vp
    n = 64                                              # (the launches that are accepted walk: a wavefront's worth of queries is enough)
    cap = 1 << 16
    d_e = mem.alloc(8 * cap + 64); d_cnt = mem.alloc(4 * n + 64); d_tot = mem.alloc(64); d_off = mem.alloc(8 * (n + 1) + 64)
    d_ql = mem.alloc(12 * n + 64); d_tl = mem.alloc(12 * c.tris.shape[0] + 64); d_first = mem.alloc(4 * n + 64)
    mem.zero(d_off, 8 * (n + 1) + 64); mem.zero(d_ql, 12 * n + 64); mem.zero(d_tl, 12 * c.tris.shape[0] + 64); mem.zero(d_tot, 64); mem.zero(d_first, 4 * n + 64)
    rec = {shape: c.dev[shape].d_records for shape in OL.SHAPES}

    def box(g=grid, tris=c.d_tris, q=rec["box"], num=n, offsets=d_off, counts=d_cnt, entries=d_e, capacity=cap, counters=0, flags=0, ctx=mem._ctx, **_):
        return L.hagrid_box_refs(ctx, G.pod(g), vp(tris), vp(q), num, vp(offsets), vp(counts), vp(entries), capacity, vp(counters), flags)

    def tri(g=grid, tris=c.d_tris, q=rec["contact"], num=n, first=0, ql=0, tl=0, offsets=d_off, counts=d_cnt, entries=d_e, capacity=cap, counters=0, flags=0, ctx=mem._ctx):
        return L.hagrid_tri_refs(ctx, G.pod(g), vp(tris), vp(q), num, vp(first), vp(ql), vp(tl), vp(offsets), vp(counts), vp(entries), capacity, vp(counters), flags)

    def obb(g=grid, tris=c.d_tris, q=rec["obb"], num=n, ql=0, tl=0, offsets=d_off, counts=d_cnt, entries=d_e, capacity=cap, counters=0, flags=0, ctx=mem._ctx, **_):
        return L.hagrid_obb_refs(ctx, G.pod(g), vp(tris), vp(q), num, vp(ql), vp(tl), vp(offsets), vp(counts), vp(entries), capacity, vp(counters), flags)

    g2 = api.build_all(mem, c.d_tris, c.tris.shape[0])
    for f, records, labelled in ((box, rec["box"], False), (tri, rec["contact"], True), (obb, rec["obb"], True)):
        assert f(counters=d_tot) == 0                                       # (every room is 0: the offsets are zeros)
        assert f(offsets=0, entries=0, capacity=0) == 0                     # count mode
        assert f(g=None) == EINVAL and f(tris=0) == EINVAL and f(q=0) == EINVAL and f(num=-1) == EINVAL and f(capacity=-1) == EINVAL
        for flags in (1, 2, 1 << 31):
            assert f(flags=flags) == EINVAL and b"flag" in L.hagrid_last_error(mem._ctx)
        assert f(offsets=0) == EINVAL and f(offsets=0, entries=0) == EINVAL and f(offsets=0, entries=0, capacity=0, counts=0) == EINVAL
        assert f(entries=0) == EINVAL and f(entries=0, capacity=0) == 0 and f(counts=0) == 0
        assert f(tris=c.d_tris + 4) == EINVAL and f(q=records + 8, num=n - 1) == EINVAL
        assert f(entries=d_e + 4) == EINVAL and f(offsets=d_off + 4) == EINVAL and f(counts=d_cnt + 2) == EINVAL and f(counters=d_tot + 4) == EINVAL
        if labelled:
            assert f(ql=d_ql, tl=d_tl) == 0
            assert f(ql=d_ql) == EINVAL and f(tl=d_tl) == EINVAL
            assert f(ql=d_ql + 2, tl=d_tl) == EINVAL and f(ql=d_ql, tl=d_tl + 2) == EINVAL
        assert f(num=0, tris=0, q=0, offsets=0, counts=0, entries=0, capacity=0) == 0
        assert f(ctx=None) == EINVAL
        shift = g2.pod.shift
        g2.pod.shift = 16
        assert f(g=g2) == EINVAL and b"shift" in L.hagrid_last_error(mem._ctx)
        g2.pod.shift = shift
    assert tri(first=d_first) == 0 and tri(first=d_first + 2) == EINVAL
    with pytest.raises(api.HagridError, match="aligned"):
        api.box_refs(grid, c.d_tris, rec["box"] + 4, 8, counts=d_cnt)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c, g2) as released:
        if released is not None:
            for name, fn, f in (("box", api.box_refs, box), ("contact", api.tri_refs, tri), ("obb", api.obb_refs, obb)):
                with pytest.raises(api.HagridError, match="released"):
                    fn(g2, c.d_tris, rec[name], n, counts=d_cnt)
                assert f(g=g2, num=0) == EINVAL
    mem.synchronize()
    for p in (d_e, d_cnt, d_tot, d_off, d_ql, d_tl, d_first):
        mem.free(p)
    api.setup_traversal(grid)
    for shape in OL.SHAPES:
        OL.assert_csr_equal(OL.device_lists(c, grid, c.dev[shape], 256, 2048), OL.csr_slice(c.want[shape], np.arange(2048, 2048 + 256)), f"{shape} {c.name} after the refused calls")


def test_kernel_budget():
    G.kernel_budget(G.kernel_listing(), one_each=("overlap_refs_kernel", "expand_select"))
