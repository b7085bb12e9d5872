"""Deep and unfinished grids on the device (tests/_deep_grids.py): the construction of grids 10 to 16 levels deep against the CPU oracle after every pass;
every consumer of the construction format -- nearest hit (variants 1 and 2, any-hit, barycentrics), multi-hit, crossing counts and lists, inside votes,
closest points, box overlap, contact queries -- after build, merge, flatten, expand and compress, against the host walk over the downloaded grid (records and
batch totals) and against the brute force; the traversal image on unflattened maps of 10 and 12 levels and its absence at virtual resolution 65536; the blob
at 15 levels; the refusal of 16 levels by every consumer.  Bit for bit; every compared output comes from a poisoned, guarded buffer (tests/_poison.py)."""
import ctypes as C

import numpy as np
import pytest

from hagrid_amd import scene

import _closest as K
import _crossing_lists as CL
import _crossings as X
import _deep_grids as D
import _multi_hit as M
import _overlap as V
import _overlap_tris as T
import _poison as P
from test_build_gpu import assert_same_grid
from test_traverse_gpu import _check_records, _expected_records, _walk_meets_link

pytestmark = pytest.mark.gpu

HAGRID_EINVAL = -1


@pytest.fixture(scope="module")
def mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    return D.build_hosts(tmp_path_factory.mktemp("deep_grids_hosts_gpu"))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)


def both_at(mem, name, tris, d_tris, stage):
    """(device stages, oracle stages) of a catalogue scene advanced to `stage`"""
    from hagrid_amd import api
    dev, orc = D.DeviceStages(name, api, mem, d_tris, tris.shape[0]), D.OracleStages(name, tris)
    for st in D.STAGES[:D.STAGES.index(stage) + 1]:
        D.stage_grid(dev, st); D.stage_grid(orc, st)
    return dev, orc


def traverse(mem, grid, d_tris, d_rays, n, flags=0):
    from hagrid_amd import api
    d_hits = P.alloc_out(mem, 16 * n)
    api.traverse_grid(grid, d_tris, d_rays, d_hits, n, flags)
    mem.synchronize()
    hits = P.fetch(mem, d_hits, api.HIT_DTYPE, n)
    mem.free(d_hits)
    return hits


def assert_hits(got, want, what):
    bad = (words(got) != words(want)).any(axis=1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} rays differ, first at {np.flatnonzero(bad)[:5]}: got {got[bad][:2]}, want {want[bad][:2]}"


# ---- a. construction ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(D.CATALOGUE))
def test_every_stage_equals_the_oracle(mem, name):
    """all five scenes, every pass; compress answers what the oracle's answers and a refusal leaves the descriptor as it was.  s15 and s16 run with every
    option at its default; that their merge works on the 32-byte records is inferred from their virtual resolution of 65536 or more (merge.hip decides by
    it; no counter tells the mode), which is what the assertion on dims << shift pins"""
    tris = D.make_tris(name)
    d_tris = mem.upload(tris)
    from hagrid_amd import api
    dev, orc = D.DeviceStages(name, api, mem, d_tris, tris.shape[0]), D.OracleStages(name, tris)
    for stage in D.STAGES[:-1]:
        grid, G = D.stage_grid(dev, stage), D.stage_grid(orc, stage)
        assert_same_grid(grid.download(mem), G, f"{name} {stage}")
        assert grid.shift == D.CATALOGUE[name]["shift"]
    assert (max(grid.dims) << grid.shift >= 65536) == (name in ("s15", "s16"))
    before = (grid.entries, grid.cells, grid.ref_ids, grid.small_cells, grid.summary())
    (grid, ok), (G, want) = D.stage_grid(dev, "compress"), D.stage_grid(orc, "compress")
    assert ok == want == D.CATALOGUE[name]["compress"]
    if not ok:
        assert (grid.entries, grid.cells, grid.ref_ids, grid.small_cells, grid.summary()) == before and not grid.small_cells
    assert_same_grid(grid.download(mem), G, f"{name} compress")
    assert grid.summary() == G.summary()
    grid.free(); mem.free(d_tris)


def test_s15_merge_compacting_throughout(mem):
    """merge.inplace = 0 on the 32-byte working records"""
    from hagrid_amd import api
    tris = D.make_tris("s15")
    d_tris = mem.upload(tris)
    try:
        mem.set_option("merge.inplace", 0)
        dev, orc = both_at(mem, "s15", tris, d_tris, "merge")
        assert_same_grid(dev.grid.download(mem), orc.grid, "s15 merge, compacting")
        assert mem.build_counts()["merged_cells"] == orc.grid.num_cells
    finally:
        mem.set_option("merge.inplace", 1)
    dev.grid.free(); mem.free(d_tris)


# ---- b. every consumer at every stage ---------------------------------------------------------------------------------------------------------------

CASES = [(name, stage) for name in D.WALKED for stage in D.stages_of(name)]


@pytest.mark.parametrize("name,stage", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_every_consumer(mem, hosts, name, stage):
    from hagrid_amd import api
    from oracle import oracle as O
    s = D.brute_answers(hosts, name)
    d = hosts["dir"]
    what = f"{name} {stage}"
    n = D.NUM_RAYS
    d_tris = mem.upload(s.tris)
    dev, orc = both_at(mem, name, s.tris, d_tris, stage)
    grid, G = dev.grid, orc.grid
    arrays = grid.download(mem)
    assert_same_grid(arrays, G, what)
    assert bool(grid.small_cells) == (stage == "compress")
    d_rays = mem.upload(s.rays)
    # (against the brute force: D.compared leaves out the rays on which the HOST walk over these same arrays differs from it -- none on s10 and s12, a
    # bounded few on s15 and nested, each with a crossing that only the reference's slack accepts; the device equals the host walk on EVERY ray)
    try:
        # nearest hit on the construction format: the reference-shaped kernel and v2; any-hit; barycentrics
        want, _ = G.traverse(s.tris, s.rays)
        mem.set_option("traverse.image", 0)
        api.setup_traversal(grid)
        for variant in (1, 2):
            mem.set_option("traverse.variant", variant)
            got = traverse(mem, grid, d_tris, d_rays, n)
            assert_hits(got, want, f"{what} variant={variant}")
            assert (got["u"] == 0).all() and (got["v"] == 0).all()
            for flags, oflags in ((api.ANY_HIT, O.ANY_HIT), (api.UVS, O.UVS)) if variant == 2 else ():       # (with a flag every launch is v2's)
                assert_hits(traverse(mem, grid, d_tris, d_rays, n, flags), G.traverse_ex(s.tris, s.rays, oflags), f"{what} variant={variant} flags={flags}")
        mem.set_option("traverse.variant", 0)
        sure = D.compared(name, (words(want) != words(s.hits)).any(axis=1), s.slack, what + ": nearest hit", nearest=True)
        assert_hits(got[sure], s.hits[sure], what + ": nearest hit against the brute force")
        assert (got["id"] >= 0).sum() >= n // 2
        # multi-hit
        for k in (1, 8):
            d_hits = P.alloc_out(mem, 16 * n * k)
            api.traverse_grid_multi(grid, d_tris, d_rays, d_hits, n, k)
            mem.synchronize()
            got = P.fetch(mem, d_hits, api.HIT_DTYPE, n * k).reshape(n, k)
            mem.free(d_hits)
            walk = M.host_walk(hosts["multi"], d, arrays, s.tris, s.rays, k)
            assert (words(got) == words(walk)).all(), f"{what}: multi-hit k={k} against the host walk"
            sure = D.compared(name, (walk["id"] != s.multi[0][:, :k]).any(axis=1) | (M.bits(walk["t"]) != M.bits(s.multi[1][:, :k])).any(axis=1), s.slack, f"{what}: multi-hit k={k}")
            assert (got["id"][sure] == s.multi[0][sure, :k]).all() and (M.bits(got["t"][sure]) == M.bits(s.multi[1][sure, :k])).all(), f"{what}: multi-hit k={k} against the brute force"
        # crossing counts, with the four totals
        d_rec = P.alloc_out(mem, 16 * n); d_tot = mem.alloc(32); mem.zero(d_tot, 32)
        api.count_crossings(grid, d_tris, d_rays, d_rec, n, d_tot)
        mem.synchronize()
        rec = P.fetch(mem, d_rec, np.uint32, 4 * n).reshape(n, 4); tot = mem.download(d_tot, np.int64, 4)
        mem.free(d_rec); mem.free(d_tot)
        walk = X.host_query(hosts["crossings"], d, s.tris, grid=arrays, page=8, rays=s.rays)
        X.assert_records_equal(rec, walk["records"], what + ": crossing records against the host walk")
        assert tot.tolist() == walk["totals"].tolist() and (tot > 0).all() and walk["excess"] <= 0
        sure = D.compared(name, (X.rec_bits(walk["records"]) != X.rec_bits(s.records)).any(axis=1), s.slack, what + ": crossing records")
        X.assert_records_equal(rec[sure], s.records[sure], what + ": crossing records against the brute force")
        # crossing lists, CSR, from the device's own counts, with the six totals
        counts = rec[:, 0].astype(np.int64)
        offsets = np.zeros(n + 1, np.int64); np.cumsum(counts, out=offsets[1:])
        cap = int(offsets[-1])
        d_ent = P.alloc_out(mem, 8 * cap); d_rec = P.alloc_out(mem, 16 * n); d_off = mem.upload(offsets); d_tot = mem.alloc(48); mem.zero(d_tot, 48)
        api.list_crossings(grid, d_tris, d_rays, n, d_ent, cap, offsets=d_off, records=d_rec, counters=d_tot)
        mem.synchronize()
        slots = P.fetch(mem, d_ent, np.uint32, 2 * cap).reshape(-1, 2); rec2 = P.fetch(mem, d_rec, np.uint32, 4 * n).reshape(n, 4); tot = mem.download(d_tot, np.int64, 6)
        mem.free(d_ent); mem.free(d_rec); mem.free(d_off); mem.free(d_tot)
        walk = CL.host_lists(hosts["lists"], d, s.tris, s.rays, cap, offsets=offsets, grid=arrays, page=8)
        assert (slots[:, 0] == walk["t"]).all() and (slots[:, 1].view(np.int32) == walk["key"]).all(), what + ": crossing lists against the host walk"
        assert (rec2 == rec).all() and tot.tolist() == walk["totals"].tolist() and tot[4] == cap and tot[5] == 0
        P.assert_all_written(slots)
        # ray by ray against the brute force's lists, each laid out by its own offsets
        sure = D.compared(name, D.lists_differ(walk, offsets, s.lists, s.offsets), s.slack, what + ": crossing lists")
        got = {"t": slots[:, 0], "key": slots[:, 1].view(np.int32)}
        bad = D.lists_differ(got, offsets, s.lists, s.offsets) & sure
        assert not bad.any(), f"{what}: the crossing lists of {bad.sum()} rays differ from the brute force, first at {np.flatnonzero(bad)[:5]}"
        if name == "nested":
            deep_rays_against_the_host_walk(mem, hosts, api, s, grid, G, arrays, d_tris, what)
        # inside votes, three directions, with the records
        m = D.NUM_POINTS
        d_pts = mem.upload(s.points)
        d_in = P.alloc_out(mem, 4 * m); d_rec = P.alloc_out(mem, 16 * m * 3); d_tot = mem.alloc(32); mem.zero(d_tot, 32)
        api.points_inside(grid, d_tris, d_pts, m, d_in, None, d_rec, d_tot)
        mem.synchronize()
        inside = P.fetch(mem, d_in, np.int32, m); prec = P.fetch(mem, d_rec, np.uint32, 4 * m * 3).reshape(m * 3, 4); tot = mem.download(d_tot, np.int64, 4)
        mem.free(d_in); mem.free(d_rec); mem.free(d_tot)
        walk = X.host_query(hosts["crossings"], d, s.tris, grid=arrays, page=8, points=s.points)
        X.assert_records_equal(prec, walk["records"], what + ": point records against the host walk")
        assert (inside == walk["inside"]).all() and tot.tolist() == walk["totals"].tolist()
        psure = D.compared(name, (X.rec_bits(walk["records"]) != X.rec_bits(s.inside["records"])).any(axis=1), s.point_slack, what + ": inside votes", points=True)
        X.assert_records_equal(prec[psure], s.inside["records"].reshape(-1)[psure], what + ": point records against the brute force")
        whole = psure.reshape(-1, 3).all(axis=1)
        assert (inside == s.inside["inside"])[whole].all() and whole.sum() >= m // 2, what + ": inside votes against the brute force"
        # closest points
        d_res = P.alloc_out(mem, 32 * m); d_tot = mem.alloc(32); mem.zero(d_tot, 32)
        api.closest_points(grid, d_tris, d_pts, d_res, m, d_tot)
        mem.synchronize()
        got = P.fetch(mem, d_res, api.CLOSEST_DTYPE, m); tot = mem.download(d_tot, np.int64, 4)
        mem.free(d_res); mem.free(d_tot); mem.free(d_pts)
        walk, wc = K.host_walk(hosts["closest"], d, arrays, s.tris, s.points)
        K.assert_results_equal(got, walk, what + ": closest points against the host walk")
        assert tot.tolist() == [m, int(wc[:, 0].sum()), int(wc[:, 1].sum()), int(wc[:, 2].sum())]
        K.assert_results_equal(got, s.closest, what + ": closest points against the brute force")
        # box overlap
        b = D.NUM_BOXES
        d_boxes = mem.upload(s.boxes)
        for k, flags in ((1, 0), (8, 0), (1, api.OVERLAP_ANY)):
            d_ids = P.alloc_out(mem, 4 * k * b); d_cnt = P.alloc_out(mem, 4 * b); d_tot = mem.alloc(32); mem.zero(d_tot, 32)
            api.overlap_boxes(grid, d_tris, d_boxes, b, k, d_ids, d_cnt, d_tot, flags)
            mem.synchronize()
            ids = P.fetch(mem, d_ids, np.int32, k * b).reshape(b, k); cnt = P.fetch(mem, d_cnt, np.int32, b); tot = mem.download(d_tot, np.int64, 4)
            mem.free(d_ids); mem.free(d_cnt); mem.free(d_tot)
            P.assert_all_written(cnt)
            w_ids, w_cnt, wt = V.host_walk(hosts["overlap"], d, arrays, s.tris, s.boxes, k, any_=bool(flags))
            V.assert_answers_equal(ids, cnt, w_ids, w_cnt, f"{what}: box overlap k={k} flags={flags} against the host walk")
            assert tot.tolist() == [b, int(wt[:, 0].astype(np.int64).sum()), int(wt[:, 1].astype(np.int64).sum()), int(wt[:, 2].astype(np.int64).sum())]
            if flags:
                member = s.overlap[8][1] > 0
                assert ((ids[:, 0] >= 0) == member).all() and (cnt == member).all(), what + ": ANY against the brute force"
            else:
                V.assert_answers_equal(ids, cnt, *s.overlap[k], f"{what}: box overlap k={k} against the brute force")
        mem.free(d_boxes)
        # contact queries
        q = s.contacts.shape[0]
        d_q = mem.upload(s.contacts)
        d_ids = P.alloc_out(mem, 4 * 8 * q); d_cnt = P.alloc_out(mem, 4 * q); d_tot = mem.alloc(32); mem.zero(d_tot, 32)
        api.overlap_tris(grid, d_tris, d_q, q, 8, d_ids, d_cnt, d_tot)
        mem.synchronize()
        ids = P.fetch(mem, d_ids, np.int32, 8 * q).reshape(q, 8); cnt = P.fetch(mem, d_cnt, np.int32, q); tot = mem.download(d_tot, np.int64, 4)
        mem.free(d_ids); mem.free(d_cnt); mem.free(d_tot); mem.free(d_q)
        P.assert_all_written(cnt)
        w_ids, w_cnt, wt = T.host_walk(hosts["contact"], d, arrays, s.tris, s.contacts, 8)
        T.assert_answers_equal(ids, cnt, w_ids, w_cnt, what + ": contact queries against the host walk")
        assert tot.tolist() == [q, int(wt[:, 0].astype(np.int64).sum()), int(wt[:, 1].astype(np.int64).sum()), int(wt[:, 2].astype(np.int64).sum())]
        T.assert_answers_equal(ids, cnt, *s.contact, what + ": contact queries against the brute force")
    finally:
        mem.set_option("traverse.variant", 0); mem.set_option("traverse.image", 2)
        mem.free(d_rays); grid.free(); mem.free(d_tris)


def deep_rays_against_the_host_walk(mem, hosts, api, s, grid, G, arrays, d_tris, what):
    """`nested`: 128 rays into the second cluster, some on through the innermost, where its voxel map is deepest and its brute force says little: the nearest hit of both kernels
    against the oracle's walk, the multi-hit lists and the crossing records with their totals against the host walks, over the same arrays, bit for bit"""
    rays = D.deep_rays(s.tris)
    n, d = rays.shape[0], hosts["dir"]
    d_rays = mem.upload(rays)
    try:
        want, _ = G.traverse(s.tris, rays)
        for variant in (1, 2):
            mem.set_option("traverse.variant", variant)
            assert_hits(traverse(mem, grid, d_tris, d_rays, n), want, f"{what} deep rays variant={variant}")
        mem.set_option("traverse.variant", 0)
        d_hits = P.alloc_out(mem, 16 * n * 8)
        api.traverse_grid_multi(grid, d_tris, d_rays, d_hits, n, 8)
        mem.synchronize()
        got = P.fetch(mem, d_hits, api.HIT_DTYPE, n * 8)
        mem.free(d_hits)
        assert (words(got) == words(M.host_walk(hosts["multi"], d, arrays, s.tris, rays, 8))).all(), what + ": deep rays, multi-hit against the host walk"
        d_rec = P.alloc_out(mem, 16 * n); d_tot = mem.alloc(32); mem.zero(d_tot, 32)
        api.count_crossings(grid, d_tris, d_rays, d_rec, n, d_tot)
        mem.synchronize()
        rec = P.fetch(mem, d_rec, np.uint32, 4 * n).reshape(n, 4); tot = mem.download(d_tot, np.int64, 4)
        mem.free(d_rec); mem.free(d_tot)
        walk = X.host_query(hosts["crossings"], d, s.tris, grid=arrays, page=8, rays=rays)
        X.assert_records_equal(rec, walk["records"], what + ": deep rays, crossing records against the host walk")
        assert tot.tolist() == walk["totals"].tolist()
        assert (rec[:, 0].view(np.int32) > 8).sum() >= n // 2, "the deep rays do not reach the inner clusters, where dozens of triangles lie on every line"
    finally:
        mem.set_option("traverse.variant", 0)
        mem.free(d_rays)


# ---- c. the traversal image ---------------------------------------------------------------------------------------------------------------------------

def sample_voxels(G, tris):
    """every voxel that holds a triangle vertex, and 4096 uniform ones"""
    res = (np.array(G.dims, np.int64) << G.shift)
    lo, hi = G.bbox_min.astype(np.float64), G.bbox_max.astype(np.float64)
    v = scene.tri_vertices(tris).reshape(-1, 3).astype(np.float64)
    at = np.clip(np.floor((v - lo) / (hi - lo) * res).astype(np.int64), 0, res - 1)
    rng = np.random.default_rng(7)
    uni = np.stack([rng.integers(0, res[c], 4096) for c in range(3)], axis=1)
    return np.ascontiguousarray(np.unique(np.concatenate([at, uni]), axis=0).astype(np.int32))


@pytest.mark.parametrize("stage", ["merge", "flatten"])
@pytest.mark.parametrize("name", ["s10", "s12", "nested"])
def test_traversal_image_layouts(mem, hosts, name, stage):
    """the general layout over maps of up to 12 single levels and over their flattened form, with and without the virtual top level: the sampled voxels
    resolve to the cells lookup_entry gives, and the image kernel (variant 4) and the default dispatch give the oracle's hits"""
    from hagrid_amd import api
    s = D.brute_answers(hosts, name)
    d_tris = mem.upload(s.tris)
    dev, orc = both_at(mem, name, s.tris, d_tris, stage)
    grid, G = dev.grid, orc.grid
    want, _ = G.traverse(s.tris, s.rays)
    vox = sample_voxels(G, s.tris)
    rec_want, begin = _expected_records(G, vox.astype(np.int64))
    d_rays = mem.upload(s.rays)
    nb = C.c_int64(0)
    try:
        for general in (1, 2):
            for vtop in (0, 1):
                mem.set_option("traverse.image_general", general); mem.set_option("traverse.image_vtop", vtop)
                api.setup_traversal(grid)
                info = mem.image_format(grid)
                assert info["general"] and mem.image_bytes(grid) > 0, (name, stage, general, vtop, info)
                recs = np.zeros((vox.shape[0], 8), np.uint32)
                assert mem._K.hagrid_kat_image_records(mem._ctx, C.byref(grid.pod), vox.ctypes.data_as(C.c_void_p), vox.shape[0], recs.ctypes.data_as(C.c_void_p), C.byref(nb)) == 0
                _, deep = _check_records(recs, rec_want, begin)
                assert (deep == _walk_meets_link(G, vox, vtop == 1)).all(), (name, stage, general, vtop)
                for variant in (0, 4):
                    mem.set_option("traverse.variant", variant)
                    assert_hits(traverse(mem, grid, d_tris, d_rays, D.NUM_RAYS), want, f"{name} {stage} general={general} vtop={vtop} variant={variant}")
    finally:
        mem.set_option("traverse.variant", 0); mem.set_option("traverse.image_general", 1); mem.set_option("traverse.image_vtop", 1)
        mem.free(d_rays); grid.free(); mem.free(d_tris)


def test_no_image_at_virtual_resolution_65536(mem, hosts):
    """s15: setup_traversal succeeds and builds nothing, traversal reads the construction format, and the grid cannot be given up for an image it has not"""
    from hagrid_amd import api
    s = D.brute_answers(hosts, "s15")
    d_tris = mem.upload(s.tris)
    dev, orc = both_at(mem, "s15", s.tris, d_tris, "expand")
    grid = dev.grid
    d_rays = mem.upload(s.rays)
    api.setup_traversal(grid)
    assert mem.image_bytes(grid) == 0 and mem.image_format(grid) == {}
    want, _ = orc.grid.traverse(s.tris, s.rays)
    assert_hits(traverse(mem, grid, d_tris, d_rays, D.NUM_RAYS), want, "s15 without an image")
    before = (grid.entries, grid.cells, grid.ref_ids, mem.usage())
    with pytest.raises(api.HagridError, match="setup_traversal"):
        api.release_for_traversal(grid)
    assert (grid.entries, grid.cells, grid.ref_ids, mem.usage()) == before
    assert_same_grid(grid.download(mem), orc.grid, "s15 after the refused release")
    mem.free(d_rays); grid.free(); mem.free(d_tris)


# ---- d. the blob at the limit ---------------------------------------------------------------------------------------------------------------------------

def test_blob_of_fifteen_levels(mem, hosts, tmp_path):
    """pack / unpack and save / load of s15 after expand: the same arrays, the same hits"""
    from hagrid_amd import api
    s = D.brute_answers(hosts, "s15")
    nt = s.tris.shape[0]
    d_tris = mem.upload(s.tris)
    dev, orc = both_at(mem, "s15", s.tris, d_tris, "expand")
    grid = dev.grid
    d_rays = mem.upload(s.rays)
    want, _ = orc.grid.traverse(s.tris, s.rays)
    p = C.c_void_p(); nb = C.c_size_t()
    api._check(mem, mem._L.hagrid_grid_pack(mem._ctx, C.byref(grid.pod), C.c_void_p(d_tris), nt, C.byref(p), C.byref(nb)), "pack")
    assert nb.value == mem._L.hagrid_grid_blob_bytes(C.byref(grid.pod), nt) > 0
    g2 = api.Grid(); g2.mem = mem
    t2 = C.c_void_p(); n2 = C.c_int()
    api._check(mem, mem._L.hagrid_grid_unpack(mem._ctx, p, nb.value, C.byref(g2.pod), C.byref(t2), C.byref(n2)), "unpack")
    path = str(tmp_path / "s15.grid")
    api._check(mem, mem._L.hagrid_grid_save(mem._ctx, C.byref(grid.pod), C.c_void_p(d_tris), nt, path.encode()), "save")
    g3, t3, n3 = api.Grid.load(mem, path)
    for g, t, k, what in ((g2, t2.value, n2.value, "unpacked"), (g3, t3, n3, "loaded")):
        assert k == nt and g.summary() == grid.summary()
        assert_same_grid(g.download(mem), orc.grid, "s15 " + what)
        assert (mem.download(t, np.float32, 12 * nt).reshape(nt, 12).view(np.uint32) == s.tris.view(np.uint32)).all()
        api.setup_traversal(g)
        assert_hits(traverse(mem, g, t, d_rays, D.NUM_RAYS), want, "s15 " + what)
        g.free(); mem.free(t)
    mem.free(d_rays); grid.free(); mem.free(d_tris)


# ---- e. sixteen levels -----------------------------------------------------------------------------------------------------------------------------------

def test_sixteen_levels_are_refused_by_every_consumer(mem, hosts, tmp_path):
    """s16 after expand: every traversal, query and blob call answers HAGRID_EINVAL with a message that names the shift, before anything is launched -- the
    outputs keep their poison and the pool its usage --, hagrid_setup_traversal included; then an ordinary construction and traversal equal the oracle's"""
    from hagrid_amd import api
    tris = D.make_tris("s16")
    nt = tris.shape[0]
    d_tris = mem.upload(tris)
    dev, orc = both_at(mem, "s16", tris, d_tris, "expand")
    grid = dev.grid
    assert grid.shift == 16 and grid.entries and grid.cells and grid.ref_ids
    assert_same_grid(grid.download(mem), orc.grid, "s16 expand")
    n = 64
    out_bytes = 16 * n * 8
    d_in = mem.upload(np.zeros((n, 12), np.float32))                 # rays, points, boxes or query triangles: nothing reads them
    d_out = P.alloc_out(mem, out_bytes); d_out2 = P.alloc_out(mem, out_bytes); d_tot = P.alloc_out(mem, 64)
    d_off = mem.upload(np.arange(n + 1, dtype=np.int64))
    L, ctx, pod = mem._L, mem._ctx, C.byref(grid.pod)
    vp = C.c_void_p
    f3 = lambda *v: (C.c_float * 3)(*v)
    blob = vp(); nbytes = C.c_size_t(); path = str(tmp_path / "s16.grid")
    calls = {
        "traverse_grid": lambda: L.hagrid_traverse_grid(ctx, pod, vp(d_tris), vp(d_in), vp(d_out), n),
        "traverse_grid_ex": lambda: L.hagrid_traverse_grid_ex(ctx, pod, vp(d_tris), vp(d_in), vp(d_out), n, api.ANY_HIT | api.UVS),
        "traverse_grid_multi": lambda: L.hagrid_traverse_grid_multi(ctx, pod, vp(d_tris), vp(d_in), vp(d_out), n, 8, 0),
        "count_crossings": lambda: L.hagrid_count_crossings(ctx, pod, vp(d_tris), vp(d_in), vp(d_out), n, vp(d_tot), 0),
        "list_crossings": lambda: L.hagrid_list_crossings(ctx, pod, vp(d_tris), vp(d_in), n, vp(d_off), 0, vp(d_out), n, vp(d_out2), vp(d_tot), 0),
        "points_inside": lambda: L.hagrid_points_inside(ctx, pod, vp(d_tris), vp(d_in), n, None, 0, vp(d_out), vp(d_out2), vp(d_tot), 0),
        "inside_lattice": lambda: L.hagrid_inside_lattice(ctx, pod, vp(d_tris), f3(0, 0, 0), f3(0.25, 0.25, 0.25), (C.c_int * 3)(4, 4, 4), None, 0, vp(d_out), vp(d_out2), vp(d_tot), 0),
        "closest_points": lambda: L.hagrid_closest_points(ctx, pod, vp(d_tris), vp(d_in), vp(d_out), n, vp(d_tot), 0),
        "overlap_boxes": lambda: L.hagrid_overlap_boxes(ctx, pod, vp(d_tris), vp(d_in), n, 8, vp(d_out), vp(d_out2), vp(d_tot), 0),
        "overlap_lattice": lambda: L.hagrid_overlap_lattice(ctx, pod, vp(d_tris), f3(0, 0, 0), f3(0.25, 0.25, 0.25), (C.c_int * 3)(4, 4, 4), 8, vp(d_out), vp(d_out2), vp(d_tot), 0),
        "overlap_tris": lambda: L.hagrid_overlap_tris(ctx, pod, vp(d_tris), vp(d_in), n, None, None, None, 8, vp(d_out), vp(d_out2), vp(d_tot), 0),
        "setup_traversal": lambda: L.hagrid_setup_traversal(ctx, pod),
        "release_for_traversal": lambda: L.hagrid_grid_release_for_traversal(ctx, pod),
        "grid_pack": lambda: L.hagrid_grid_pack(ctx, pod, vp(d_tris), nt, C.byref(blob), C.byref(nbytes)),
        "grid_save": lambda: L.hagrid_grid_save(ctx, pod, vp(d_tris), nt, path.encode()),
    }
    usage = mem.usage()
    whole = (grid.entries, grid.cells, grid.ref_ids, grid.summary())
    for name, call in calls.items():
        rc = call()
        msg = L.hagrid_last_error(ctx).decode()
        assert rc == HAGRID_EINVAL, (name, rc, msg)
        assert "shift" in msg, (name, msg)
        assert mem.usage() == usage, name
        assert (grid.entries, grid.cells, grid.ref_ids, grid.summary()) == whole, name
    mem.synchronize()
    for ptr, size in ((d_out, out_bytes), (d_out2, out_bytes), (d_tot, 64)):
        assert (P.fetch(mem, ptr, np.uint8, size) == 0xFF).all(), "a refused call wrote its output"
    assert not blob.value and mem.image_bytes(grid) == 0
    assert L.hagrid_grid_blob_bytes(pod, nt) == 0
    import os
    assert not os.path.exists(path), "a file that hagrid_grid_load would refuse"
    for ptr in (d_in, d_out, d_out2, d_tot, d_off):
        mem.free(ptr)
    grid.free(); mem.free(d_tris)
    # the context works as before
    s = D.brute_answers(hosts, "s10")
    d_tris = mem.upload(s.tris)
    dev, orc = both_at(mem, "s10", s.tris, d_tris, "expand")
    assert_same_grid(dev.grid.download(mem), orc.grid, "s10 after the refusals")
    d_rays = mem.upload(s.rays)
    api.setup_traversal(dev.grid)
    assert_hits(traverse(mem, dev.grid, d_tris, d_rays, D.NUM_RAYS), orc.grid.traverse(s.tris, s.rays)[0], "s10 after the refusals")
    mem.free(d_rays); dev.grid.free(); mem.free(d_tris)
