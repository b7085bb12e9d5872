"""Crossing lists on the GPU (hagrid_list_crossings, the list mode of the kernel of hagrid_amd/csrc/crossings.hip): the device's entries against the fixture
tests/golden/crossing_lists.npz in CSR form with offsets from the device's own counts, on Cell and SmallCell grids, with a traversal image present and ray
binning on; the stride form; rooms that are short, long and malformed; batch tails; records null and given; the six counters against the host walk's;
hostile rays and a larger live case against the host walk; api.crossing_lists from torch tensors; a C++ program through the shim; every argument error; the
kernel budget.  Every compared output comes from a poisoned, guarded buffer (tests/_poison.py); empty entries are compared exactly against (the bits of
tmax, -1), slots that no ray owns against the poison.
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import sys

import numpy as np
import pytest

import _crossing_lists as CL
import _crossings as X
import _gpu_case as G
import _multi_hit as M
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

assert P.GUARD == 8 * CL.GUARD, "the guard behind the entries is CL.GUARD slots on the host and on the device"


@pytest.fixture(scope="module")
def fixture():
    return {**np.load(X.FIXTURE), **np.load(CL.FIXTURE)}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("crossing_lists_host_gpu")
    return CL.build_host(d), d


@pytest.fixture(scope="module", params=X.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, the rays uploaded"""
    c = G.open_case(request.param, X.make_tris(request.param))
    c.rays = fixture[c.name + "_rays"]
    c.want_records = fixture[c.name + "_records"]
    c.lists = CL.fixture_lists(fixture, c.name)
    c.n = c.rays.shape[0]
    c.d_rays = c.mem.upload(c.rays)
    yield c
    c.mem.close()


def run_lists(c, grid, d_rays, n, capacity, offsets=None, stride=0, records=True, counters=True):
    """what CL.host_lists returns, from the device: "t", "key" (capacity,), "records" (n, 4) uint32 or None, "totals" int64[6]; the guard is asserted"""
    mem = c.mem
    d_ent = P.alloc_out(mem, 8 * capacity)
    d_rec = P.alloc_out(mem, 16 * n) if records else 0
    d_off = mem.upload(np.ascontiguousarray(offsets, dtype=np.int64)) if offsets is not None else 0
    d_tot = 0
    if counters:
        d_tot = mem.alloc(48); mem.zero(d_tot, 48)
    c.api.list_crossings(grid, c.d_tris, d_rays, n, d_ent, capacity, offsets=d_off, stride=stride, records=d_rec, counters=d_tot)
    mem.synchronize()
    slots = P.fetch(mem, d_ent, np.uint32, 2 * capacity).reshape(-1, 2)
    out = {"t": slots[:, 0].copy(), "key": slots[:, 1].view(np.int32).copy(), "guard": np.full((CL.GUARD, 2), CL.POISON), "records": None}
    mem.free(d_ent)
    if records:
        out["records"] = P.fetch(mem, d_rec, np.uint32, 4 * n).reshape(n, 4)
        mem.free(d_rec)
    if counters:
        out["totals"] = mem.download(d_tot, np.int64, 6)
        mem.free(d_tot)
    mem.free(d_off)
    return out


def device_offsets(c, grid, d_rays, n):
    """count, scan: the exclusive sums of the device's own counts"""
    mem = c.mem
    d_rec = P.alloc_out(mem, 16 * n)
    c.api.count_crossings(grid, c.d_tris, d_rays, d_rec, n)
    mem.synchronize()
    counts = P.fetch(mem, d_rec, np.uint32, 4 * n).reshape(n, 4)[:, 0].view(np.int32)
    mem.free(d_rec)
    o = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=o[1:])
    return o


@pytest.mark.parametrize("compress", [False, True])
def test_device_entries_equal_the_fixture(case, compress):
    """count, scan, fill: every slot written exactly once, no empty entry, every bit the fixture's; the records are crossings.npz"""
    c = case
    grid = c.grids[compress]
    c.mem.set_option("traverse.image", 0)
    try:
        o = device_offsets(c, grid, c.d_rays, c.n)
        assert (o == c.lists[0]).all()
        total = int(o[-1])
        got = run_lists(c, grid, c.d_rays, c.n, total, offsets=o)
    finally:
        c.mem.set_option("traverse.image", 2)
    want = scene.crossing_slots(o, total, c.lists, c.rays[:, 7])
    assert want["written"].all() and (want["key"] >= 0).all()
    CL.assert_slots(got, want, f"{c.name} compress={compress}")
    X.assert_records_equal(got["records"], c.want_records, f"{c.name} compress={compress}")
    assert got["totals"][0] == c.n and got["totals"][4] == total and got["totals"][5] == 0


def test_image_and_binning_are_ignored_and_survive(case):
    c = case
    grid = c.grids[False]
    total = int(c.lists[0][-1])
    want = scene.crossing_slots(c.lists[0], total, c.lists, c.rays[:, 7])
    with G.image_present(c, grid, binning=True):
        got = run_lists(c, grid, c.d_rays, c.n, total, offsets=c.lists[0])
    CL.assert_slots(got, want, f"{c.name} image present, binning on")
    X.assert_records_equal(got["records"], c.want_records, c.name)


def test_stride_form(case):
    """S = 1, 8, 9, 32: below the page, at it, one beyond, above the longest list; three slots behind the last ray's that nobody owns"""
    c = case
    for S in (1, 8, 9, 32):
        cap = c.n * S + 3
        want = scene.crossing_slots(S, cap, c.lists, c.rays[:, 7])
        for compress in (False, True):
            got = run_lists(c, c.grids[compress], c.d_rays, c.n, cap, stride=S)
            CL.assert_slots(got, want, f"{c.name} S={S} compress={compress}")
            X.assert_records_equal(got["records"], c.want_records, f"{c.name} S={S}")
    assert want["short"] == 0 and want["count"] == c.lists[0][-1]


def test_short_long_and_malformed_offsets(case):
    """every room one short, two long; a negative, a decreasing and a beyond-capacity pair write nothing; the records do not depend on the rooms"""
    c = case
    for name, offsets, cap in CL.layouts(c.lists):
        want = scene.crossing_slots(offsets, cap, c.lists, c.rays[:, 7])
        got = run_lists(c, c.grids[True], c.d_rays, c.n, cap, offsets=offsets)
        CL.assert_slots(got, want, f"{c.name} {name}")
        X.assert_records_equal(got["records"], c.want_records, f"{c.name} {name}")
        if name == "short":
            assert got["totals"][5] == (c.lists[0][1:] > c.lists[0][:-1]).sum() > 0
        if name == "malformed":
            assert not want["written"].all()


def test_batch_tails(case):
    """prefixes of 1, 63, 64 and 65 rays and the last 65 (the aimed rays with long lists), in both forms: the tail of a wavefront writes nothing"""
    c = case
    grid = c.grids[True]
    o, t, key = c.lists
    c.api.list_crossings(grid, c.d_tris, 0, 0, 0, 0, stride=1)                  # no rays: nothing is launched, null buffers are fine
    c.api.list_crossings(grid, 0, 0, 0, 0, 0, offsets=0, stride=4)
    for first, n in ((0, 1), (0, 63), (0, 64), (0, 65), (c.n - 65, 65)):
        sub = (o[first:first + n + 1] - o[first], t[o[first]:o[first + n]], key[o[first]:o[first + n]])
        rays = c.rays[first:first + n]
        total = int(sub[0][-1])
        got = run_lists(c, grid, c.d_rays + 32 * first, n, total, offsets=sub[0])
        CL.assert_slots(got, scene.crossing_slots(sub[0], total, sub, rays[:, 7]), f"{c.name} rays {first} .. {first + n}, CSR")
        X.assert_records_equal(got["records"], c.want_records[first:first + n], f"{c.name} n={n}")
        got = run_lists(c, grid, c.d_rays + 32 * first, n, 9 * n, stride=9)
        CL.assert_slots(got, scene.crossing_slots(9, 9 * n, sub, rays[:, 7]), f"{c.name} rays {first} .. {first + n}, S = 9")
        assert got["totals"][0] == n


def test_records_and_counters_null(case):
    c = case
    total = int(c.lists[0][-1])
    want = scene.crossing_slots(c.lists[0], total, c.lists, c.rays[:, 7])
    got = run_lists(c, c.grids[False], c.d_rays, c.n, total, offsets=c.lists[0], records=False, counters=False)
    assert got["records"] is None
    CL.assert_slots(got, want, f"{c.name} records and counters null")


@pytest.mark.parametrize("compress", [False, True])
def test_counters_equal_the_host_walk(case, host, compress):
    """the six batch totals, with rooms one short so that the fifth and the sixth both count; they are ADDED to"""
    c = case
    exe, d = host
    grid = c.grids[compress]
    _, offsets, cap = CL.layouts(c.lists)[1]
    got = run_lists(c, grid, c.d_rays, c.n, cap, offsets=offsets)
    w = CL.host_lists(exe, d, c.tris, c.rays, cap, offsets=offsets, grid=grid.download(c.mem), page=8)
    assert got["totals"].tolist() == w["totals"].tolist() and (got["totals"] > 0).all()
    assert (got["t"] == w["t"]).all() and (got["key"] == w["key"]).all()
    X.assert_records_equal(got["records"], w["records"], f"{c.name} compress={compress} against the host walk over the device's grid")
    mem = c.mem
    d_ent = mem.alloc(8 * cap + 8); d_off = mem.upload(offsets)
    G.assert_totals_added(lambda d_tot: c.api.list_crossings(grid, c.d_tris, c.d_rays, c.n, d_ent, cap, offsets=d_off, counters=d_tot), mem, got["totals"])
    mem.free(d_ent); mem.free(d_off)


@pytest.mark.parametrize("scene_name", ["soup", "mesh"])
def test_hostile_rays(host, scene_name):
    """the catalogue of tests/_hostile_rays.py at the grid's resolution: device = host walk over the device's grid on EVERY family, entries, records and
    counters; inadmissible rays get empty entries with the bits of their tmax"""
    import _hostile_rays as H
    from hagrid_amd import api
    exe, d = host
    tris = X.make_tris(scene_name)
    c = G.upload_case(tris); mem = c.mem
    rays, family = H.catalogue(tris, X.oracle_grid(tris, False, True), mesh=scene_name == "mesh")
    n = rays.shape[0]
    d_rays = mem.upload(rays)
    grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=True)
    o = device_offsets(c, grid, d_rays, n)
    o[1:] += 2 * np.arange(1, n + 1)                     # two slots to spare for every ray: empty entries everywhere
    cap = int(o[-1])
    got = run_lists(c, grid, d_rays, n, cap, offsets=o)
    w = CL.host_lists(exe, d, tris, rays, cap, offsets=o, grid=grid.download(mem), page=8)
    assert (got["t"] == w["t"]).all() and (got["key"] == w["key"]).all(), "device = host walk over the same grid on EVERY family"
    X.assert_records_equal(got["records"], w["records"], scene_name)
    assert got["totals"].tolist() == w["totals"].tolist() and got["totals"][5] == 0 and w["excess"] <= 0
    refused = np.flatnonzero(~H._admissible(rays))
    assert refused.size
    for i in refused[:200]:
        assert o[i + 1] - o[i] == 2 and (got["key"][o[i]:o[i + 1]] == -1).all() and (got["t"][o[i]:o[i + 1]] == M.bits(rays[i, 7])).all()
    grid.free()
    mem.free(d_rays)
    mem.close()


def test_larger_live_case(tmp_path):
    """100 000 triangles, 65 536 mixed rays (primary, incoherent, aimed through the scene, some with finite windows): count, scan, fill on the device against
    the host walk over the SAME grid arrays (downloaded), counters included, and against the numpy statement for the first 128 rays"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    lo, hi = scene.tris_bbox(tris)
    n = 65536
    rays = np.concatenate([scene.make_rays_primary(lo, hi, 128, 128), scene.make_rays_incoherent(lo, hi, 32768, 5), X.aimed_rays(tris, 16384, 6)]).astype(np.float32)
    rays[::7, 3] = np.float32(0.1); rays[::7, 7] = np.float32(0.9)
    rays = np.ascontiguousarray(rays[np.random.default_rng(5).permutation(n)])
    c = G.upload_case(tris); mem = c.mem
    d_rays = mem.upload(rays)
    exe = CL.build_host(tmp_path)
    grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=True)
    o = device_offsets(c, grid, d_rays, n)
    total = int(o[-1])
    got = run_lists(c, grid, d_rays, n, total, offsets=o)
    w = CL.host_lists(exe, tmp_path, tris, rays, total, offsets=o, grid=grid.download(mem), page=8)
    assert (got["t"] == w["t"]).all() and (got["key"] == w["key"]).all() and (got["key"] >= 0).all()
    X.assert_records_equal(got["records"], w["records"], "soup 100k against the host walk")
    assert got["totals"].tolist() == w["totals"].tolist() and w["excess"] <= 0 and got["totals"][4] == total and got["totals"][5] == 0
    m = o[1:] - o[:-1]
    assert m.max() > 16 and (m == 0).any() and (m > 8).sum() > 1000
    so, st, sk = scene.ray_crossing_lists(tris, rays[:128])
    assert (so == o[:129]).all() and (M.bits(st) == got["t"][:so[-1]]).all() and (sk == got["key"][:so[-1]]).all()
    grid.free()
    mem.close()


def test_crossing_lists_from_torch_tensors(fixture):
    """api.crossing_lists on torch's stream: the offsets are the cumsum of the counts; tri, t and entering are numpy's"""
    import torch
    from hagrid_amd import api
    tris = X.make_tris("mesh")
    rays = fixture["mesh_rays"]
    o, t, key = CL.fixture_lists(fixture, "mesh")
    mem = api.MemManager(keep=True)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_tris = torch.from_numpy(tris).cuda()
            t_rays = torch.from_numpy(rays).cuda()
            grid = api.build_all(mem, t_tris.data_ptr(), tris.shape[0])
            r = api.crossing_lists(grid, t_tris, t_rays, rays.shape[0])
            assert r["offsets"].dtype == torch.int64 and r["t"].dtype == torch.float32 and r["tri"].dtype == torch.int32 and r["entering"].dtype == torch.bool
            assert (r["offsets"][1:] == torch.cumsum(r["records"][:, 0], 0)).all() and r["offsets"][0] == 0
            got = {k: v.cpu().numpy() for k, v in r.items()}
            none = api.crossing_lists(grid, t_tris, t_rays[:0], 0)
            assert none["offsets"].tolist() == [0] and none["t"].numel() == 0
            grid.free()
        stream.synchronize()
    finally:
        mem.use_stream(None)
    mem.close()
    assert (got["offsets"] == o).all() and (M.bits(got["t"]) == M.bits(t)).all() and (got["tri"] == key >> 1).all() and (got["entering"] == ((key & 1) != 0)).all()
    X.assert_records_equal(got["records"].view(np.uint32), fixture["mesh_records"], "crossing_lists records")
    # the snippet of INTEGRATION.md: per-layer thickness = the differences of t inside a ray, layer p between entries 2p and 2p + 1
    ray = np.repeat(np.arange(rays.shape[0]), o[1:] - o[:-1])
    pos = np.arange(t.size) - o[ray]
    first = (pos % 2 == 0) & (pos + 1 < (o[1:] - o[:-1])[ray])
    thick = got["t"][np.flatnonzero(first) + 1] - got["t"][first]
    assert (thick >= 0).all() and thick.size == ((o[1:] - o[:-1]) // 2).sum()


def test_cpp_program_through_the_shim(tmp_path):
    import _subproc
    r = _subproc.check([G.build_shim("crossing_lists", tmp_path), "20000", "1000"], timeout=120)
    sys.stdout.write(r.stdout)
    assert " 0 mismatches vs host brute force" in r.stdout and " 0 mismatches in the stride form" in r.stdout, r.stdout


def test_errors_leave_the_context_working(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    n = 256
    cap = 8 * n
    d_ent = mem.alloc(8 * cap + 64); d_rec = mem.alloc(16 * n + 64); d_tot = mem.alloc(64)
    d_off = mem.upload(np.arange(n + 1, dtype=np.int64) * 8)
    EINVAL, ERANGE = G.EINVAL, G.ERANGE
    vp = G.vp

    def call(g=grid, tris=c.d_tris, rays=c.d_rays, k=n, offsets=d_off, stride=0, entries=d_ent, capacity=cap, records=d_rec, counters=d_tot, flags=0, ctx=mem._ctx):
        return L.hagrid_list_crossings(ctx, G.pod(g), vp(tris), vp(rays), k, vp(offsets), stride, vp(entries), capacity, vp(records), vp(counters), flags)

    assert call() == 0 and call(offsets=0, stride=8) == 0 and call(records=0, counters=0) == 0
    # a null context, a null grid, null buffers
    assert call(ctx=None) == EINVAL
    assert call(g=None) == EINVAL and b"grid" in L.hagrid_last_error(mem._ctx)
    assert call(tris=0) == EINVAL and call(rays=0) == EINVAL and call(entries=0) == EINVAL and b"null" in L.hagrid_last_error(mem._ctx)
    assert call(entries=0, capacity=0) == 0, "no capacity: no entries needed, every room is 0"
    # misaligned buffers
    assert call(tris=c.d_tris + 4) == EINVAL and call(rays=c.d_rays + 8) == EINVAL and call(records=d_rec + 8) == EINVAL
    assert call(offsets=d_off + 4) == EINVAL and call(entries=d_ent + 4) == EINVAL and call(counters=d_tot + 4) == EINVAL
    assert b"aligned" in L.hagrid_last_error(mem._ctx)
    # counts and capacity
    assert call(k=-1) == EINVAL and call(capacity=-1) == EINVAL and b"capacity" in L.hagrid_last_error(mem._ctx)
    # both or neither of offsets and stride >= 1
    assert call(stride=8) == EINVAL and call(offsets=0) == EINVAL and call(offsets=0, stride=-1) == EINVAL and call(stride=-3) == EINVAL
    assert b"stride" in L.hagrid_last_error(mem._ctx)
    # any flag
    for flags in (1, 2, 1 << 31):
        assert call(flags=flags) == EINVAL and b"flag" in L.hagrid_last_error(mem._ctx)
    # num_rays * stride beyond the capacity
    assert call(offsets=0, stride=9) == ERANGE and call(offsets=0, stride=8, capacity=cap - 1) == ERANGE and b"capacity" in L.hagrid_last_error(mem._ctx)
    assert call(offsets=0, stride=(1 << 31) - 1, k=(1 << 31) - 1) == ERANGE, "the product is taken in 64 bits"
    assert call(k=0, rays=0, tris=0, entries=0, capacity=0) == 0
    with pytest.raises(api.HagridError, match="aligned"):
        api.list_crossings(grid, c.d_tris, c.d_rays + 4, 8, d_ent, cap, stride=8)
    with pytest.raises(api.HagridError, match="capacity"):
        api.list_crossings(grid, c.d_tris, c.d_rays, n, d_ent, cap, stride=9)
    # "traverse.id_is_steps" = 1
    mem.set_option("traverse.id_is_steps", 1)
    try:
        with pytest.raises(api.HagridError, match="id_is_steps"):
            api.list_crossings(grid, c.d_tris, c.d_rays, n, d_ent, cap, stride=8)
    finally:
        mem.set_option("traverse.id_is_steps", 0)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.list_crossings(g2, c.d_tris, c.d_rays, n, d_ent, cap, stride=8)
            assert call(g=g2, k=0) == EINVAL
    mem.free(d_ent); mem.free(d_rec); mem.free(d_tot); mem.free(d_off)
    total = int(c.lists[0][-1])
    got = run_lists(c, grid, c.d_rays, c.n, total, offsets=c.lists[0])
    CL.assert_slots(got, scene.crossing_slots(c.lists[0], total, c.lists, c.rays[:, 7]), f"{c.name} after the refused calls")
    X.assert_records_equal(got["records"], c.want_records, f"{c.name} after the refused calls")


def test_kernel_budget():
    """the list mode is a mode of the one crossings kernel, not a kernel of its own"""
    from hagrid_amd import lib
    assert "hagrid_list_crossings" in lib.SIGNATURES
    G.kernel_budget(G.kernel_listing(), one_each=("crossings_kernel",))         # crossing queries are ONE kernel
