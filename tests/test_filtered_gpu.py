"""Filtered traversal on the GPU (hagrid_traverse_grid_filtered, a mode of the kernel of hagrid_amd/csrc/trav_multi.hip): the device's lists against the
brute force scene.filtered_hits (ids equal, t bit-equal, no ray excepted) and against the multi-hit fixture with the filter laid over it; the null
combinations, and no filter at all against hagrid_traverse_grid_multi bit for bit; any-hit; rays that start on their triangle; edges; every refusal;
MeshScene.instance_masks; one deep grid and a larger live case against the filtered host walk over the downloaded grid arrays.  Outputs are poisoned and
guarded (tests/_poison.py).
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import ctypes as C

import numpy as np
import pytest

import _filtered as F
import _gpu_case as G
import _multi_hit as M
from _poison import alloc_out, fetch
from hagrid_amd import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=F.SCENES)
def case(request):
    """one scene of the fixture: Cell and SmallCell grids built on the device; rays, filters and triangle masks uploaded"""
    inp = F.inputs(request.param)
    c = G.open_case(request.param, inp.tris)
    c.mem.set_option("traverse.image", 0)                         # (read by setup_traversal alone: building the grids does not look at it)
    c.inp, c.rays, c.n = inp, inp.rays, inp.n
    c.d_rays = c.mem.upload(c.rays)
    c.d_filters = c.mem.upload(c.inp.filters)
    c.d_masks = c.mem.upload(c.inp.tri_masks)
    yield c
    c.mem.close()


def run(c, grid, d_rays, n, k, d_filters=0, d_masks=0, flags=0, multi=False, d_tris=None):
    """the lists of n rays as an (n, k) HIT_DTYPE array out of a poisoned buffer whose guard must stay untouched; multi: hagrid_traverse_grid_multi"""
    mem = c.mem
    d_hits = alloc_out(mem, 16 * n * k)
    d_tris = c.d_tris if d_tris is None else d_tris
    if multi:
        c.api.traverse_grid_multi(grid, d_tris, d_rays, d_hits, n, k, flags)
    else:
        c.api.traverse_grid_filtered(grid, d_tris, d_rays, d_hits, n, k, d_filters, d_masks, flags)
    mem.synchronize()
    got = fetch(mem, d_hits, c.api.HIT_DTYPE, n * k)            # (an untouched record reads t = NaN: no comparison of t bits passes on it)
    mem.free(d_hits)
    return got.reshape(n, k)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def combo_ptrs(c, combo):
    f, m = F.COMBOS[combo]
    return (c.d_filters if f else 0), (c.d_masks if m else 0)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("compress", [False, True])
def test_device_lists_equal_the_statement(case, compress, k):
    c = case
    F.assert_filter_bites(c.inp)
    got = run(c, c.grids[compress], c.d_rays, c.n, k, c.d_filters, c.d_masks)
    ids, t = F.wanted(c.name, "both")
    F.assert_lists(got, ids, t, f"{c.name} compress={compress} k={k}")
    assert (got["u"] == 0).all() and (got["v"] == 0).all()
    # the fixture (the reference's arithmetic) with the filter laid over its eight slots, wherever those decide
    f_ids, f_t, decided = F.from_fixture(c.inp, k, c.inp.filters, c.inp.tri_masks)
    assert (~decided).sum() <= F.UNDECIDED_CAP[c.name]
    F.assert_lists(got, f_ids, f_t, f"{c.name} compress={compress} k={k} against the fixture", only=decided)


@pytest.mark.parametrize("compress", [False, True])
def test_null_combinations_and_all_ones(case, compress):
    c = case; mem = c.mem
    grid = c.grids[compress]
    for combo in ("filters", "masks", "neither"):
        d_f, d_m = combo_ptrs(c, combo)
        ids, t = F.wanted(c.name, combo)
        for k in (1, 8):
            F.assert_lists(run(c, grid, c.d_rays, c.n, k, d_f, d_m), ids, t, f"{c.name} compress={compress} {combo} k={k}")
    # no filter at all, and all-ones masks with skip -1: hagrid_traverse_grid_multi bit for bit, u and v included
    d_ones_f = mem.upload(F.all_ones_filters(c.n))
    d_ones_m = mem.upload(np.full(c.tris.shape[0], 0xFFFFFFFF, dtype=np.uint32))
    for k in (1, 8):
        for flags in (0, c.api.UVS):
            want = run(c, grid, c.d_rays, c.n, k, flags=flags, multi=True)
            assert (words(run(c, grid, c.d_rays, c.n, k, 0, 0, flags)) == words(want)).all(), f"{c.name} k={k} flags={flags}: no filters"
            assert (words(run(c, grid, c.d_rays, c.n, k, d_ones_f, d_ones_m, flags)) == words(want)).all(), f"{c.name} k={k} flags={flags}: all-ones filters"
        assert not F.lists_differ(want["id"], want["t"], c.inp.ids[:, :k], c.inp.t[:, :k]).any()
    mem.free(d_ones_f); mem.free(d_ones_m)


@pytest.mark.parametrize("compress", [False, True])
def test_any_hit(case, compress):
    """id >= 0 exactly where the k = 1 list is not empty; (id, t) a candidate of that ray; with UVS u and v the oracle's for the reported pair"""
    from oracle import oracle as O
    c = case
    grid = c.grids[compress]
    for combo in F.COMBOS:
        d_f, d_m = combo_ptrs(c, combo)
        f, m = F.combo_args(c.inp, combo)
        got = run(c, grid, c.d_rays, c.n, 1, d_f, d_m, c.api.ANY_HIT)[:, 0]
        F.assert_any_hit(got, c.tris, c.rays, f, m, F.wanted(c.name, combo)[0][:, 0], f"{c.name} compress={compress} {combo} any-hit")
        assert (got["u"] == 0).all() and (got["v"] == 0).all()
    got = run(c, grid, c.d_rays, c.n, 1, c.d_filters, c.d_masks, c.api.ANY_HIT | c.api.UVS)[:, 0]
    F.assert_any_hit(got, c.tris, c.rays, c.inp.filters, c.inp.tri_masks, F.wanted(c.name, "both")[0][:, 0], f"{c.name} compress={compress} any-hit with uvs")
    L = O.lib()
    tris = np.ascontiguousarray(c.tris, dtype=np.float32); rays = np.ascontiguousarray(c.rays, dtype=np.float32)
    h = np.zeros(1, dtype=O.HIT_DTYPE)
    hit = np.flatnonzero(got["id"] >= 0)
    assert hit.size >= F.MIN_NON_EMPTY
    nonzero = 0
    for i in hit:
        tid = int(got["id"][i])
        assert L.orc_intersect_prim_ray_uv(tris[tid].ctypes.data_as(C.c_void_p), rays[i].ctypes.data_as(C.c_void_p), tid, h.ctypes.data_as(C.c_void_p)) == 1
        assert words(h["t"])[0] == words(got["t"][i:i + 1])[0] and words(h["u"])[0] == words(got["u"][i:i + 1])[0] and words(h["v"])[0] == words(got["v"][i:i + 1])[0]
        nonzero += int(h["u"][0] != 0 or h["v"][0] != 0)
    assert nonzero > hit.size // 2
    assert (got["u"][got["id"] < 0] == 0).all() and (got["v"][got["id"] < 0] == 0).all()


def test_rays_that_start_on_their_triangle(case):
    """origin = the hit point of a primary ray, tmin = 0, a mirrored direction, skip = that triangle through api.skip_filters: no epsilon.  Without the skip
    at least a quarter of these rays report the triangle they start on in slot 0 -- the reason the feature exists."""
    import torch
    c = case; api, mem = c.api, c.mem
    rays, own = F.self_exclusion_rays(c.inp)
    m = rays.shape[0]
    assert m > 500
    plain_ids, _ = scene.filtered_hits(c.tris, rays, 4)
    self_hits = int((plain_ids[:, 0] == own).sum())
    print(f"{c.name}: {self_hits} of {m} rays report their own triangle in slot 0 without a skip")
    assert self_hits * 4 >= m
    hits = np.zeros(m, dtype=scene.HIT_DTYPE); hits["id"] = own
    t_hits = torch.from_numpy(hits.view(np.int32).reshape(m, 4).copy()).cuda()
    torch.cuda.synchronize()
    t_filters = api.skip_filters(t_hits, mem=mem)
    assert t_filters.shape == (m, 2) and t_filters.dtype == torch.int32
    mem.synchronize()
    f = t_filters.cpu().numpy()
    assert (f[:, 0] == -1).all() and (f[:, 1] == own).all()
    d_rays = mem.upload(rays)
    want_ids, want_t = scene.filtered_hits(c.tris, rays, 4, f, None)
    assert not (want_ids == own[:, None]).any() and (want_ids[:, 0] >= 0).sum() > 20
    for compress in (False, True):
        got = run(c, c.grids[compress], d_rays, m, 4, t_filters.data_ptr())
        F.assert_lists(got, want_ids, want_t, f"{c.name} compress={compress} rays on their triangle")
        occ = run(c, c.grids[compress], d_rays, m, 1, t_filters.data_ptr(), 0, api.ANY_HIT)[:, 0]
        F.assert_any_hit(occ, c.tris, rays, f, None, want_ids[:, 0], f"{c.name} compress={compress} occlusion rays")
    # another mask: the low 31 bits and the top bit survive the int32 tensor
    t2 = api.skip_filters(t_hits, mask=0x80000001, mem=mem)
    mem.synchronize()
    assert (t2.cpu().numpy()[:, 0].view(np.uint32) == 0x80000001).all()
    mem.free(d_rays)


def test_edges(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    ids, t = F.wanted(c.name, "both")
    api.traverse_grid_filtered(grid, c.d_tris, 0, 0, 0, 4)                       # no rays: nothing is launched, null buffers are fine
    api.traverse_grid_filtered(grid, c.d_tris, 0, 0, 0, 1, c.d_filters, c.d_masks, api.ANY_HIT)
    # batches that are no multiple of 64, at an offset into the ray buffer; the filters move with the rays; nothing beyond num_rays * k records (the guard)
    for n, first in ((1, 0), (63, 5), (1000, 64), (4095, 1)):
        got = run(c, grid, c.d_rays + 32 * first, n, 5, c.d_filters + 8 * first, c.d_masks)
        F.assert_lists(got, ids[first:first + n], t[first:first + n], f"{c.name} n={n} first={first}")
    # rays with mask 0 and inactive rays among live ones; a skip >= the number of triangles
    rays = c.rays[:640].copy()
    rays[::3] = scene.make_rays_inactive(rays[::3].shape[0])
    f = c.inp.filters[:640].copy()
    f[1::3, 0] = 0
    f[2::6, 1] = c.tris.shape[0] + np.arange(f[2::6].shape[0]) * 1000003 % (1 << 30)
    assert (f[2::6, 1] >= c.tris.shape[0]).all()
    d_r = mem.upload(rays); d_f = mem.upload(f)
    want_ids, want_t = scene.filtered_hits(c.tris, rays, 8, f, c.inp.tri_masks)
    for compress in (False, True):
        got = run(c, c.grids[compress], d_r, 640, 8, d_f, c.d_masks)
        F.assert_lists(got, want_ids, want_t, f"{c.name} compress={compress} mask 0 and inactive rays among live ones")
        assert (got["id"][::3] == -1).all() and (got["t"][::3] == np.float32(-1.0)).all()
        assert (got["id"][1::3] == -1).all() and (M.bits(got["t"][1::3]) == M.bits(np.repeat(rays[1::3, 7:8], 8, axis=1))).all()
        assert (got["u"] == 0).all() and (got["v"] == 0).all()
    # the rays next to them are unaffected: a skip that names no triangle is no skip
    live = np.arange(640) % 3 == 2
    f_live = c.inp.filters[:640].copy(); f_live[2::6, 1] = -1
    l_ids, l_t = scene.filtered_hits(c.tris, c.rays[:640], 8, f_live, c.inp.tri_masks)
    assert not F.lists_differ(want_ids[live], want_t[live], l_ids[live], l_t[live]).any() and (want_ids[live, 0] >= 0).sum() > 30
    mem.free(d_r); mem.free(d_f)


def test_prefix_property(case):
    c = case
    full = run(c, c.grids[True], c.d_rays, c.n, 8, c.d_filters, c.d_masks, c.api.UVS)
    for k in (1, 3, 7):
        got = run(c, c.grids[True], c.d_rays, c.n, k, c.d_filters, c.d_masks, c.api.UVS)
        assert (words(got) == words(np.ascontiguousarray(full[:, :k]))).all()


def test_errors_leave_the_context_working(case):
    import _deep_grids as D
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    d_hits = alloc_out(mem, 16 * 8 * c.n)
    call = lambda *a, **kw: api.traverse_grid_filtered(grid, c.d_tris, c.d_rays, d_hits, *a, **kw)
    # the nearest-hit path before
    mem.set_option("traverse.image", 2)
    api.setup_traversal(grid)
    d_near = mem.alloc(16 * c.n)

    def nearest():
        mem.one(d_near, 16 * c.n)
        api.traverse_grid(grid, c.d_tris, c.d_rays, d_near, c.n)
        mem.synchronize()
        return mem.download(d_near, api.HIT_DTYPE, c.n)

    before = nearest()
    state = mem.order_state(c.d_rays)
    for k in (0, -1, 9, 1 << 20):
        with pytest.raises(api.HagridError, match="HAGRID_MAX_HITS"):
            call(c.n, k, c.d_filters, c.d_masks)
    for flags in (4, 8, 4 | api.UVS, 1 << 31):
        with pytest.raises(api.HagridError, match="unknown flag"):
            call(c.n, 1, c.d_filters, c.d_masks, flags)
    for k in (2, 8):
        with pytest.raises(api.HagridError, match="ANY_HIT needs k = 1"):
            call(c.n, k, c.d_filters, c.d_masks, api.ANY_HIT)
    with pytest.raises(api.HagridError, match="aligned"):
        call(c.n - 1, 4, c.d_filters + 4, c.d_masks)
    for off in (1, 2):
        with pytest.raises(api.HagridError, match="aligned"):
            call(c.n - 1, 4, c.d_filters, c.d_masks + off)
    with pytest.raises(api.HagridError, match=r"failed \(-4\)"):                         # HAGRID_ERANGE: the range check comes before any launch
        call((1 << 31) - 1, 2, c.d_filters, c.d_masks)
    mem.set_option("traverse.id_is_steps", 1)
    try:
        with pytest.raises(api.HagridError, match="id_is_steps"):
            call(c.n, 4, c.d_filters, c.d_masks)
    finally:
        mem.set_option("traverse.id_is_steps", 0)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:                                # ("traverse.image" is 2 already)
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.traverse_grid_filtered(g2, c.d_tris, c.d_rays, d_hits, c.n, 4, c.d_filters, c.d_masks)
    # the level limit of make_args: a grid sixteen levels deep
    deep = D.make_tris("s16")
    d_deep = mem.upload(deep)
    dev = D.DeviceStages("s16", api, mem, d_deep, deep.shape[0])
    for st in D.stages_of("s16"):
        D.stage_grid(dev, st)
    assert dev.grid.shift == 16
    with pytest.raises(api.HagridError, match="shift"):
        api.traverse_grid_filtered(dev.grid, d_deep, c.d_rays, d_hits, 64, 4, c.d_filters, 0)
    dev.grid.free(); mem.free(d_deep)
    mem.synchronize()
    assert (fetch(mem, d_hits, np.uint8, 16 * 8 * c.n) == 0xFF).all(), "a refused call wrote its output"
    mem.free(d_hits)
    # afterwards a correct launch runs, and the nearest-hit path has not moved
    ids, t = F.wanted(c.name, "both")
    got = run(c, grid, c.d_rays, c.n, 8, c.d_filters, c.d_masks)
    F.assert_lists(got, ids, t, f"{c.name} after the refused calls")
    assert mem.order_state(c.d_rays) == state, "the hints of the nearest-hit path moved"
    after = nearest()
    mem.free(d_near)
    assert (words(before) == words(after)).all()
    mem.set_option("traverse.image", 0)
    api.setup_traversal(grid)


def test_instance_masks():
    """two meshes, three instances assembled on the device; every ray carries a set of instance bits; the masks repeated per instance in numpy"""
    import torch
    from hagrid_amd import api
    soups = [scene.make_soup(3000, seed=21), scene.make_soup(2000, seed=22)]
    verts = [np.ascontiguousarray(scene.tri_vertices(s).reshape(-1, 3), np.float32) for s in soups]
    instance_mesh = [0, 1, 0]
    transforms = np.zeros((3, 3, 4), dtype=np.float32)
    transforms[:, [0, 1, 2], [0, 1, 2]] = 1.0
    transforms[1, :, 3] = (0.25, 0.0, 0.125); transforms[2, :, 3] = (0.0, 0.375, -0.25)
    mem = api.MemManager(keep=True)
    c = G.Case(); c.api, c.mem = api, mem
    tv = [torch.from_numpy(v).cuda() for v in verts]
    tt = torch.from_numpy(transforms.reshape(3, 12)).cuda()
    torch.cuda.synchronize()
    ms = api.MeshScene(mem, [(tv[0].data_ptr(), verts[0].shape[0], 0, 3000), (tv[1].data_ptr(), verts[1].shape[0], 0, 2000)], instance_mesh)
    n_tris = ms.num_tris
    assert n_tris == 8000 and ms.num_instances == 3
    c.d_tris = mem.alloc(48 * n_tris)
    ms.assemble(tt.data_ptr(), c.d_tris)
    inst_masks = [1, 2, 0x80000000]
    t_masks = ms.instance_masks(inst_masks)
    assert t_masks.shape == (n_tris,) and t_masks.dtype == torch.int32
    with pytest.raises(ValueError):
        ms.instance_masks([1, 2])
    grid = api.build_all(mem, c.d_tris, n_tris)
    mem.synchronize()
    tris = mem.download(c.d_tris, np.float32, 12 * n_tris).reshape(n_tris, 12)
    want_masks = np.repeat(np.asarray(inst_masks, dtype=np.uint32), [3000, 2000, 3000])
    assert (t_masks.cpu().numpy().view(np.uint32) == want_masks).all()
    lo, hi = scene.tris_bbox(tris)
    rays = np.concatenate([scene.make_rays_primary(lo, hi, 32, 32), scene.make_rays_incoherent(lo, hi, 1024, 9)]).astype(np.float32)
    n = rays.shape[0]
    subsets = np.asarray([1, 2, 0x80000000, 3, 0x80000001, 0x80000002, 0x80000003], dtype=np.uint32)
    f = np.empty((n, 2), dtype=np.int32)
    f[:, 0] = subsets[np.arange(n) % 7].view(np.int32); f[:, 1] = -1
    d_rays = mem.upload(rays); d_f = mem.upload(f)
    want_ids, want_t = scene.filtered_hits(tris, rays, 8, f, want_masks)
    plain_ids, _ = scene.filtered_hits(tris, rays, 8)
    got = run(c, grid, d_rays, n, 8, d_f, t_masks.data_ptr())
    F.assert_lists(got, want_ids, want_t, "three instances, one bit each")
    assert (want_ids[:, 0] >= 0).sum() > 300 and (want_ids[:, 0] != plain_ids[:, 0]).sum() > 100
    first = np.asarray([ms.first_tri(i) for i in range(4)])
    rows, cols = np.nonzero(want_ids >= 0)
    instance = np.searchsorted(first, want_ids[rows, cols], side="right") - 1
    assert ((f[rows, 0].view(np.uint32) & np.asarray(inst_masks, np.uint32)[instance]) != 0).all(), "every listed triangle belongs to an instance the ray sees"
    ms.close(); grid.free(); mem.close()


def test_one_deep_grid(tmp_path):
    """scene s12, final stage (compressed, twelve levels): the device's lists equal the filtered host walk over the downloaded arrays, no ray excepted"""
    import _deep_grids as D
    from hagrid_amd import api
    name = "s12"
    tris = D.make_tris(name)
    rays = D.make_rays(name, tris)
    n = rays.shape[0]
    c = G.upload_case(tris); mem = c.mem
    dev = D.DeviceStages(name, api, mem, c.d_tris, tris.shape[0])
    for st in D.stages_of(name):
        D.stage_grid(dev, st)
    grid = dev.grid
    assert grid.shift == D.CATALOGUE[name]["shift"] and grid.small_cells
    arrays = grid.download(mem)
    exe = F.build_host(tmp_path)
    plain = F.host_walk(exe, tmp_path, arrays, tris, rays, 8)
    filters = F.make_filters(n, tris.shape[0], plain["id"][:, 0], plain["id"][:, 1])
    masks = F.tri_masks(tris.shape[0])
    d_rays = mem.upload(rays); d_f = mem.upload(filters); d_m = mem.upload(masks)
    want = {k: F.host_walk(exe, tmp_path, arrays, tris, rays, k, filters, masks) for k in (1, 8)}
    for k in (1, 8):
        got = run(c, grid, d_rays, n, k, d_f, d_m)
        assert (words(got) == words(want[k])).all(), f"{name} k={k}"
    assert (want[8]["id"][:, 0] >= 0).sum() > n // 4 and (want[8]["id"][:, 0] != plain["id"][:, 0]).sum() > n // 10
    occ = run(c, grid, d_rays, n, 1, d_f, d_m, api.ANY_HIT)[:, 0]
    F.assert_any_hit(occ, tris, rays, filters, masks, want[1]["id"][:, 0], f"{name} any-hit")
    grid.free(); mem.close()


def test_larger_live_case(tmp_path):
    """100 000 triangles, 16 384 rays (primary and incoherent mixed, every fifth with a finite window), k = 8, both cell formats: the device's lists against
    the filtered host walk over the SAME grid arrays (downloaded)"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    rays = M.mixed_rays(tris, 96, 96, 7168)
    rays = np.ascontiguousarray(rays[np.random.default_rng(5).permutation(rays.shape[0])])      # both kinds of rays in every wavefront
    n = rays.shape[0]
    assert n == 16384
    c = G.upload_case(tris); mem = c.mem
    d_rays = mem.upload(rays)
    masks = F.tri_masks(tris.shape[0])
    d_m = mem.upload(masks)
    exe = F.build_host(tmp_path)
    filters = None
    for compress in (False, True):
        grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=compress)
        arrays = grid.download(mem)
        if filters is None:
            plain = run(c, grid, d_rays, n, 2, multi=True)
            filters = F.make_filters(n, tris.shape[0], plain["id"][:, 0], plain["id"][:, 1])
            d_f = mem.upload(filters)
        got = run(c, grid, d_rays, n, 8, d_f, d_m)
        want = F.host_walk(exe, tmp_path, arrays, tris, rays, 8, filters, masks)
        assert (words(got) == words(want)).all(), f"soup 100k compress={compress} against the host walk"
        hist = M.hit_histogram(want["id"])
        assert hist[0] > 0 and hist[8] > 0, "the batch has rays without a candidate and rays with full lists"
        assert (want["id"][:, 0] != plain["id"][:, 0]).sum() > n // 20
        grid.free()
    mem.close()
