"""The branches a pass takes only when a count crosses a constant, when an optional buffer is missing or when a counter wraps -- none of which an input of the
other files' sizes reaches:

  by inputs alone      more than 2048 large primitives (build.hip: their workgroups stride over the list); more distance tasks than resident wavefronts and more
                       triangles than the size mode's launch (distance.hip: grid-stride loops); more than 524 288 references without a traversal image
                       (trav_image.hip: max_ref_kernel strides); expansions of 17 .. 33 iterations (expand.hip: the listed passes end at 48); whole
                       constructions under ctx.fast_readback = 0 and scan.lookback = 2
  by selectors         (csrc/kat/hagrid_amd_kat.h, host side only) distance.by_triangle: the splat over triangles; expand.listed / expand.max_listed: no list, and
                       the switch back to all-cells passes while thousands of cells still grow; scan.epoch: the look-back status words restart their epochs

Every test asserts the condition that puts its input on the branch, from the input itself, from what the library reports (build counts, query counters, device
info) or from the epoch read back; the conditions that need no GPU are in test_fallbacks_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import _distance as D
import _fallbacks as F
from _poison import alloc_out, fetch
from hagrid_amd import scene
from test_build_gpu import assert_same_grid, run_stages
from test_distance_lattice_gpu import assert_equal, run_distance, small_case
from test_scan_gpu import TILE, scan

pytestmark = pytest.mark.gpu

EINVAL = -1
EPOCH_END = (1 << 30) - 2           # ctx.hip lookback_state: the epochs restart once this one has been used


@pytest.fixture(scope="module")
def mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


def traverse_equals_oracle(mem, grid, G, d_tris, tris, num_rays, seed):
    from hagrid_amd import api
    rays = scene.make_rays_incoherent(G.bbox_min, G.bbox_max, num_rays, seed)
    d_rays = mem.upload(rays); d_hits = alloc_out(mem, 16 * num_rays)
    api.traverse_grid(grid, d_tris, d_rays, d_hits, num_rays)
    hits = fetch(mem, d_hits, api.HIT_DTYPE, num_rays)
    want, _ = G.traverse(tris, rays, nthreads=8)
    assert (hits["id"] == want["id"]).all() and (hits["t"].view(np.uint32) == want["t"].view(np.uint32)).all()
    assert (want["id"] >= 0).mean() > 0.05
    mem.free(d_rays); mem.free(d_hits)
    return want


# ---- 1: more than 2048 large primitives --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", F.NEEDLE_COUNTS)
def test_more_large_primitives_than_their_workgroups(mem, m):
    """count_top_refs / emit_top_refs give the primitives whose box covers 64 top-level cells or more min(their number, 2048) workgroups: with 2049 and 3000 of
    them the workgroups stride over the list (b += gridDim.x - first_big_block), with 2048 every workgroup has exactly one.  Every stage against the oracle, then
    50 000 incoherent rays."""
    tris = F.needle_scene(m)
    grid, G, d_tris = run_stages(mem, tris)
    large = F.large_primitives(tris, G.dims, G.bbox_min, G.bbox_max)          # the reach condition, from the input and the grid's dims
    assert large >= m and (large > F.BIG_BLOCKS) == (m > F.BIG_BLOCKS), (large, G.dims)
    assert mem.build_counts()["num_tris"] == 2000 + m
    want = traverse_equals_oracle(mem, grid, G, d_tris, tris, 50000, 5)
    assert (want["id"] >= 2000).any(), "no ray meets a needle"
    grid.free(); mem.free(d_tris)


# ---- 2, 6: the distance lattice -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def whole_lattice():
    """the case whose every box is the whole lattice, on the device, with the numpy statement of its answers (made once)"""
    tris, origin, size, n, band = F.whole_lattice_case()
    c = small_case(tris)
    c.origin, c.size, c.n, c.band = origin, size, n, band
    c.want = scene.distance_lattice(tris, origin, size, n, band)
    c.want.setflags(write=False)
    yield c
    c.grid.free(); c.mem.close()


def test_more_distance_tasks_than_resident_wavefronts(whole_lattice):
    """12 800 tasks on a launch of 32 wavefronts per compute unit: the splat's loop over tasks strides (t += gridDim.x)"""
    c = whole_lattice
    got = run_distance(c, c.grid, c.origin, c.size, c.n, c.band)
    assert_equal(got, c.want, "every box the whole lattice")
    t = got["totals"].tolist()
    assert [t[0], t[1], t[3]] == [200, 12800, 131072], t
    assert t[1] > 32 * c.mem.device_info()["compute_units"]                    # the reach condition
    assert (c.want["id"] >= 0).all() and np.unique(c.want["id"]).size == 200


def by_triangle_cases(whole_lattice):
    """(what, case on the device, origin, size, n, band, the numpy statement's records, pairs within the band) of every case with several tasks per triangle"""
    fx = dict(np.load(D.FIXTURE))
    out = []
    tris, origin, size, n = D.case("boxes_c")
    boxes = small_case(tris)
    for band in (0.75, 2.5, 0.0):
        out.append((f"boxes_c band {band}", boxes, origin, size, n, band, scene.distance_lattice(tris, origin, size, n, band), D.pairs_within(tris, origin, size, n, band)))
    v = np.float32([[0.0, 0.0, 0.0], [1.0, 0.2, 0.1], [0.1, 1.0, 0.3]])
    one = small_case(scene.tris_from_vertices(v[0:1], v[1:2], v[2:3]))
    origin, size, n = np.float32([-0.35, -0.3, -0.45]), np.float32([0.07, 0.09, 0.11]), (23, 17, 11)
    for band in (0.1, 5.0):
        want = scene.distance_lattice(one.tris, origin, size, n, band)
        out.append((f"one triangle band {band}", one, origin, size, n, band, want, int((want["id"] >= 0).sum())))
    tris, origin, size, n = D.case("solids_a")
    solids = small_case(tris)
    out.append(("solids_a band 3 voxels", solids, origin, size, n, D.band_of(size, 3.0), D.fixture_records(fx, "solids_a", 1), int(fx["solids_a_pairs"][1])))
    c = whole_lattice               # (a band of 4 on a scene 1.4 across: every triangle is within the band of every centre)
    out.append(("every box the whole lattice", c, c.origin, c.size, c.n, c.band, c.want, 200 * 131072))
    return out, (boxes, one, solids)


def test_splat_by_triangles(whole_lattice):
    """distance.by_triangle = 1 sets the word a sum of task counts beyond 31 bits leaves (no real input can: 2^30 tasks are 2^41 voxel tests): the splat's loop
    runs over triangles, each with all the runs of its box.  Every output and all four counters are those of the splat by tasks and of the numpy statement -- the
    pairs counter too: both modes offer every triangle the same voxels.  (No counter tells the modes apart: the reach condition is the selector itself, which
    the product's hagrid_set_option refuses.)"""
    cases, own = by_triangle_cases(whole_lattice)
    try:
        for what, c, origin, size, n, band, want, pairs in cases:
            runs = {}
            for by_tri in (0, 1):
                c.mem.set_option("distance.by_triangle", by_tri)
                runs[by_tri] = got = run_distance(c, c.grid, origin, size, n, band)
                assert_equal(got, want, f"{what}, by_triangle {by_tri}")
            a, b = runs[0], runs[1]
            assert (a["totals"] == b["totals"]).all(), (what, a["totals"], b["totals"])
            assert (a["ids"] == b["ids"]).all() and (a["d2"].view(np.uint32) == b["d2"].view(np.uint32)).all()
            assert (a["records"].view(np.uint32) == b["records"].view(np.uint32)).all()
            assert a["totals"][2] == pairs and a["totals"][3] == (want["id"] >= 0).sum(), (what, a["totals"], pairs)
            if what in ("boxes_c band 0.75", "boxes_c band 2.5", "one triangle band 5.0", "every box the whole lattice"):
                assert a["totals"][1] >= 2 * a["totals"][0] > 0, (what, a["totals"])        # several tasks per triangle: by triangles a wavefront takes runs one after the other
    finally:
        for _, c, *_ in cases:
            c.mem.set_option("distance.by_triangle", 0)
    for c in own:
        c.grid.free(); c.mem.close()


# ---- 3: more triangles than the size mode's launch, more references than max_ref_kernel's --------------------------------------------------

def test_more_triangles_than_the_size_launch_and_no_traversal_image(mem, tmp_path):
    """64 * 32 * compute_units + 4097 triangles: the size mode's lanes stride over the triangles (distance.hip); more than 524 288 references and no traversal
    image: hagrid_distance_lattice asks max_ref_kernel for the triangle count, whose 2048 workgroups stride over the references.  Against the host program's
    definition over all pairs (the counters of triangles with a box and of tasks against the host's scatter); then with the image's count: the same answer."""
    from hagrid_amd import api
    cus = mem.device_info()["compute_units"]
    if cus > 512:
        pytest.skip("more than 512 compute units: the scene that crosses the launch would be too large for a quick test")
    N = 64 * 32 * cus + 4097
    tris = scene.make_soup(N)
    c = type("Case", (), {})()
    c.api, c.mem, c.tris = api, mem, tris
    c.d_tris = mem.upload(tris)
    grid = api.build_all(mem, c.d_tris, N)                 # no setup_traversal: the context holds no image of this grid
    assert mem.image_bytes(grid) == 0
    assert grid.num_refs > 524288 and N > 64 * 32 * cus    # the reach conditions
    origin, size, n = np.float32([0.31, 0.27, 0.42]), np.float32([0.05, 0.045, 0.04]), (6, 5, 4)
    band = D.band_of(size, 1.5)
    exe = D.build_host(tmp_path)
    box = (grid.bbox_min, grid.bbox_max)
    want, cw = D.host_distance(exe, tmp_path, tris, origin, size, n, band, "brute", grid_box=box)
    _, cs = D.host_distance(exe, tmp_path, tris, origin, size, n, band, "scatter", grid_box=box)
    totals = [int(cs[0]), int(cs[1]), int(cw[2]), int(cw[3])]
    assert cs[2] == cw[2] and cs[3] == cw[3] and totals[0] > 1000 and totals[3] == 120
    got = run_distance(c, grid, origin, size, n, band)
    assert_equal(got, want, "528k triangles, no image")
    assert got["totals"].tolist() == totals, (got["totals"], totals)
    api.setup_traversal(grid)
    assert mem.image_bytes(grid) > 0
    again = run_distance(c, grid, origin, size, n, band)
    assert_equal(again, want, "528k triangles, the image's count")
    assert again["totals"].tolist() == totals
    grid.free(); mem.free(c.d_tris)


# ---- 4, 7: the expansion ------------------------------------------------------------------------------------------------------------------

class Expansion:
    """one scene's grid before its expansion, on the device and in the oracle; run() expands a fresh copy of it"""

    def __init__(self, mem, name):
        from hagrid_amd import api
        self.mem, self.api = mem, api
        self.tris, td, sd, alpha = F.expand_scene(name)
        _, G = F.oracle_before_expansion(name)
        self.d_tris = mem.upload(self.tris)
        self.grid = api.Grid()
        api.build_grid(mem, self.d_tris, self.tris.shape[0], self.grid, td, sd)
        api.merge_grid(mem, self.grid, alpha); api.flatten_grid(mem, self.grid)
        assert_same_grid(self.grid.download(), G, "before the expansion")
        self.fresh = G.cells.copy()
        self.n = self.fresh.shape[0]

    def run(self, iters):
        mem, grid = self.mem, self.grid
        mem.copy_h2d(grid.cells, self.fresh)
        # (best effort: the pool of a `keep` manager hands the pass the buffers the previous expansion gave back, with its -- correct -- cells still in them)
        spare = [alloc_out(mem, 32 * self.n, guard=0) for _ in range(2)]
        for p in spare: mem.free(p)
        self.api.expand_grid(mem, grid, self.d_tris, iters)
        assert mem.build_counts()["expand_passes"] == 3 * iters
        return mem.download(grid.cells, scene.CELL_DTYPE, self.n)

    def close(self):
        self.grid.free(); self.mem.free(self.d_tris)


def assert_same_cells(got, want, what):
    for f in ("min", "max", "begin", "end"):
        bad = (got[f] != want[f]).reshape(got.shape[0], -1).any(axis=1)
        assert not bad.any(), f"{what}: {f} differs in {bad.sum()} of {bad.size} cells, first at {np.flatnonzero(bad)[:5]}: got {got[f][bad][:3]}, want {want[f][bad][:3]}"


@pytest.mark.parametrize("subset_only", [1, 0])
@pytest.mark.parametrize("name", ["soup4000", "soup333_fine"])
def test_expansion_beyond_the_listed_passes_as_the_product_runs_it(mem, name, subset_only):
    """17 iterations end on the last listed pass (48 = 3 * 16), 18 and more leave the listed passes for the all-cells pass in mid-sequence.  Nothing grows
    there any more (the last iteration that changes a cell is the 12th on these scenes, the 16th at most on any scene measured: the voxel map's extent bounds
    the growth), so this pins the parity of the two cell buffers and the pointer the grid gets back, nothing else; the switch while cells still grow is
    test_the_switch_to_all_cells_passes_in_the_middle_of_growth."""
    sweep = [(17, 1), (18, 1), (18, 0), (19, 1), (33, 1)]
    E = F.oracle_expansions(name, [k for k, _ in sweep], bool(subset_only))
    x = Expansion(mem, name)
    try:
        mem.set_option("expand.subset_only", subset_only)
        for iters, voxel_map in sweep:
            mem.set_option("expand.voxel_map", voxel_map)
            assert_same_cells(x.run(iters), E[iters], f"{name} subset_only {subset_only} iters {iters} voxel_map {voxel_map}")
    finally:
        mem.set_option("expand.subset_only", 1); mem.set_option("expand.voxel_map", 1)
    x.close()


@pytest.mark.parametrize("subset_only", [1, 0])
@pytest.mark.parametrize("name", sorted(F.EXPAND_SCENES))
def test_the_switch_to_all_cells_passes_in_the_middle_of_growth(mem, name, subset_only):
    """expand.max_listed puts the end of the listed passes (three per iteration from the second on) into the iterations where hundreds to ten thousands of
    cells still change: 0 = never listed, 3 / 6 / 9 = all-cells passes again from the third / fourth / fifth iteration, 47 = the list's counts one short of
    their room.  A listed pass stores only the cells it looked at and relies on the other buffer being the one of two passes ago; the all-cells pass that
    follows must find both buffers complete.  expand.listed = 0 is the expansion whose optional list could not be allocated."""
    iters = (2, 3, 4, 5, 8)
    E = F.oracle_expansions(name, iters, bool(subset_only))
    assert F.cells_differ(E[3], E[2]) >= 100 and F.cells_differ(E[4], E[3]) >= 100 and F.cells_differ(E[5], E[4]) > 0      # still growing where the switch falls
    x = Expansion(mem, name)
    try:
        mem.set_option("expand.subset_only", subset_only)
        for max_listed in (0, 3, 6, 9, 47):
            mem.set_option("expand.max_listed", max_listed)
            for k in iters:
                assert_same_cells(x.run(k), E[k], f"{name} subset_only {subset_only} max_listed {max_listed} iters {k}")
        mem.set_option("expand.max_listed", 48); mem.set_option("expand.listed", 0)
        for k in (2, 5):
            assert_same_cells(x.run(k), E[k], f"{name} subset_only {subset_only} without the list, iters {k}")
    finally:
        mem.set_option("expand.subset_only", 1); mem.set_option("expand.max_listed", 48); mem.set_option("expand.listed", 1)
    x.close()


# ---- 5: hooks no test set -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fast_readback,lookback", [(0, 1), (1, 2), (0, 2)])
def test_whole_construction_with_plain_readbacks_and_helping_scans(mem, fast_readback, lookback):
    """ctx.fast_readback = 0: every scalar the construction reads back comes by hipMemcpyAsync + hipStreamSynchronize; scan.lookback = 2: every scan of the
    construction helps at its first miss.  build, merge, flatten, expand and compress against the oracle, then 20 000 incoherent rays."""
    tris = scene.make_soup(30000, seed=91)
    try:
        mem.set_option("ctx.fast_readback", fast_readback); mem.set_option("scan.lookback", lookback)
        grid, G, d_tris = run_stages(mem, tris)
        traverse_equals_oracle(mem, grid, G, d_tris, tris, 20000, 9)
    finally:
        mem.set_option("ctx.fast_readback", 1); mem.set_option("scan.lookback", 1)
    grid.free(); mem.free(d_tris)


# ---- 8: the epochs of the look-back status words restart --------------------------------------------------------------------------------------

def test_lookback_epochs_restart():
    """scan.epoch puts a fresh context a few scans before the end of its epochs (2^30 - 2: 2^30 scans in one context, a service that lives for days): the scans
    that cross the restart -- alone, and in the middle of a construction -- give numpy's / the oracle's answers, and the epoch read back has started again."""
    from hagrid_amd import api
    mem = api.MemManager(keep=True)
    rng = np.random.default_rng(31)
    sizes = (65 * TILE + 77, 1_000_003)

    def check_scan(it):
        words, n, in_place = 1 + (it & 1), sizes[(it >> 1) & 1], 4 * ((it >> 2) & 1)
        v = rng.integers(0, 9, size=(n, words), dtype=np.int32)
        out, total = scan(mem, v.reshape(-1), words, None, 1 | in_place)
        incl = np.cumsum(v.astype(np.int64), axis=0)
        assert (out.reshape(n, words)[1:] == incl[:-1]).all() and (out.reshape(n, words)[0] == 0).all() and (total == incl[-1]).all(), it

    assert mem.scan_epoch() == 0
    for it in (2, 3):
        check_scan(it)                       # (the status words grow to the largest scan's size here: growing restarts the epochs too, and must not stand in for the wrap)
    start = EPOCH_END - 4
    mem.set_option("scan.epoch", start)
    assert mem.scan_epoch() == start
    epochs = []
    for it in range(12):
        check_scan(it)
        epochs.append(mem.scan_epoch())
    assert epochs[:4] == [start + 1, start + 2, start + 3, EPOCH_END], epochs[:5]
    assert epochs[4:] == list(range(1, 9)), epochs                     # the restart happened, once, behind the last epoch
    assert mem.scan_epoch() < start

    # a whole construction across the restart
    tris = scene.make_soup(30000, seed=91)
    grid, G, d_tris = run_stages(mem, tris)                            # (the status words grow to the construction's sizes)
    grid.free()
    before = mem.scan_epoch()
    grid, G, d_tris2 = run_stages(mem, tris)
    grid.free(); mem.free(d_tris2)
    per_construction = mem.scan_epoch() - before
    assert per_construction > 8, "a construction is dozens of scans"
    mem.set_option("scan.epoch", start)
    grid, G, d_tris2 = run_stages(mem, tris)
    assert 0 < mem.scan_epoch() < per_construction                   # restarted behind its first scans, in the middle of a pass
    traverse_equals_oracle(mem, grid, G, d_tris2, tris, 20000, 9)
    grid.free(); mem.free(d_tris2); mem.free(d_tris)

    # only forwards
    now = mem.scan_epoch()
    assert now > 0
    assert mem._K.hagrid_kat_set_option(mem._ctx, b"scan.epoch", now - 1) == EINVAL
    assert mem._K.hagrid_kat_set_option(mem._ctx, b"scan.epoch", -1) == EINVAL and mem._K.hagrid_kat_set_option(mem._ctx, b"scan.epoch", (1 << 30) + 1) == EINVAL
    assert mem.scan_epoch() == now
    mem.set_option("scan.epoch", now)
    mem.close()


# ---- the selectors are not options of the product ---------------------------------------------------------------------------------------------

def test_the_product_refuses_the_selectors(mem):
    L, K = mem._L, mem._K
    for key, good, bad in ((b"distance.by_triangle", 0, 2), (b"expand.listed", 1, 2), (b"expand.max_listed", 48, 49), (b"scan.epoch", mem.scan_epoch(), -1)):
        assert L.hagrid_set_option(mem._ctx, key, good) == EINVAL and b"unknown key" in L.hagrid_last_error(mem._ctx), key
        assert K.hagrid_kat_set_option(mem._ctx, key, bad) == EINVAL, key
        assert K.hagrid_kat_set_option(mem._ctx, key, good) == 0, key
    assert K.hagrid_kat_set_option(mem._ctx, b"expand.max_listed", -1) == EINVAL
    assert K.hagrid_kat_scan_epoch(mem._ctx, None) == EINVAL and K.hagrid_kat_scan_epoch(None, C.byref(C.c_int32())) == EINVAL
