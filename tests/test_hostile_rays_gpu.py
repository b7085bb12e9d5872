"""The traversal kernels on the hostile-ray catalogue (tests/_hostile_rays.py), embedded in batches of ordinary rays: every kernel variant gives the CPU
oracle's records bit for bit, the fixture's (the reference brute force's id / t) on the families that are in general position to the scene, the contract's
record for every inadmissible ray, the records of the +0 family for the -0 family, and leaves the records behind the hit buffer alone."""
import functools

import numpy as np
import pytest

import _hostile_rays as H
import _multi_hit as M
from _poison import alloc_out, fetch
from _traverse_formats import IMAGE_FORMATS, image_scenes

pytestmark = pytest.mark.gpu

CASES = [(name, grid, compress) for name in H.SCENES for grid in H.GRID_PARAMS for compress in (False, True)]
IDS = [f"{n}-{g}-{'small' if c else 'cell'}" for n, g, c in CASES]
DEFAULT_CASES = [c for c in CASES if c[1] == "default"]
DEFAULT_IDS = [i for c, i in zip(CASES, IDS) if c[1] == "default"]
PAD = 4


def words(hits) -> np.ndarray:
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4)


@pytest.fixture(scope="module")
def mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


class World:
    """a scene, an oracle grid, its catalogue embedded in a batch, and what the oracle says about the batch"""

    def __init__(self, tris, G, fixture=None, mesh=None):
        from oracle import oracle as O
        self.tris, self.G = tris, G
        self.cat, self.fam = H.catalogue(tris, G, mesh=mesh)
        self.rays, self.pos = H.embed(self.cat, G.bbox_min, G.bbox_max)
        self.n = self.rays.shape[0]
        O.walk_capped()
        self.want, self.stats, self.steps = G.traverse(tris, self.rays, want_steps=True)
        with O.walk_mode(O.DEVICE_F2I):          # the conversions the device performs: the catalogue must not depend on them
            dev_want, dev_stats, dev_steps = G.traverse(tris, self.rays, want_steps=True)
        assert O.walk_capped() == (0, -1)
        assert (words(dev_want) == words(self.want)).all() and dev_stats == self.stats and (dev_steps == self.steps).all()
        self.fixture = fixture
        self.inadmissible = ~H._admissible(self.rays)
        assert (self.inadmissible[self.pos] == (self.fam == "j")).all() and self.inadmissible.sum() == (self.fam == "j").sum()

    def check(self, got, what, uvs=None, ids=True):
        """got: the device's records of the batch.  uvs: the oracle's records with barycentrics (None: u = v = 0 everywhere)"""
        g, w = words(got), words(self.want if uvs is None else uvs)
        cols = slice(0, 4) if ids else slice(1, 4)
        bad = (g[:, cols] != w[:, cols]).any(axis=1)
        assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} records differ from the oracle's, first at {np.flatnonzero(bad)[:5]}: got {got[bad][:2]}, want {self.want[bad][:2]}"
        if uvs is None:
            assert (g[:, 2:4] == 0).all(), what
        if not ids:
            return
        assert (g[self.inadmissible] == H.contract_records(self.rays[self.inadmissible])).all(), f"{what}: an inadmissible ray's record"
        c = got[self.pos]
        assert (words(c[self.fam == "a"]) == words(c[self.fam == "b"])).all(), f"{what}: the -0 family against the +0 family"
        if self.fixture is not None:
            general = np.isin(self.fam, list("abcdefgh"))
            assert (words(c[general])[:, 0:2] == words(self.fixture[general])[:, 0:2]).all(), f"{what}: the reference brute force's id / t"


@functools.lru_cache(maxsize=None)
def _world(name, grid, compress):
    tris = H.make_tris(name)
    G = H.oracle_grid(tris, H.GRID_PARAMS[grid], compress)
    w = World(tris, G)
    w.fixture = H.fixture_hits(np.load(H.FIXTURE), name, grid, w.cat)
    return w


class Device:
    """a world on the device: triangles, grid, the batch in a ray buffer"""

    def __init__(self, mem, w):
        from hagrid_amd import api
        self.api, self.mem, self.w = api, mem, w
        G = w.G
        self.d_tris = mem.upload(w.tris)
        self.grid = api.Grid.upload(mem, G.entries, G.ref_ids, G.cells, G.small_cells, G.bbox_min, G.bbox_max, G.dims, G.shift, G.offsets)
        self.d_rays = mem.upload(w.rays)

    def run(self, flags=0, d_rays=None, n=None, k=0):
        """nearest-hit (k = 0) or multi-hit traversal into a buffer PAD records longer than needed; those must stay untouched"""
        mem, n = self.mem, self.w.n if n is None else n
        d_rays = self.d_rays if d_rays is None else d_rays
        count = n * max(k, 1)
        d_hits = mem.alloc(16 * (count + PAD)); mem.one(d_hits, 16 * (count + PAD))
        if k:
            self.api.traverse_grid_multi(self.grid, self.d_tris, d_rays, d_hits, n, k, flags)
        else:
            self.api.traverse_grid(self.grid, self.d_tris, d_rays, d_hits, n, flags)
        mem.synchronize()
        got = mem.download(d_hits, self.api.HIT_DTYPE, count + PAD)
        mem.free(d_hits)
        assert (got[count:].view(np.uint32) == 0xFFFFFFFF).all(), "written beyond the hit buffer"
        return got[:count]

    def close(self):
        self.mem.free(self.d_rays); self.grid.free(); self.mem.free(self.d_tris)


def _only_inadmissible(dev, what, k=0):
    """a batch that holds nothing but inadmissible rays (its length no multiple of 64)"""
    w = dev.w
    bad = w.rays[w.inadmissible][:-1] if w.inadmissible.sum() % 64 == 0 else w.rays[w.inadmissible]
    d = dev.mem.upload(bad)
    try:
        got = dev.run(d_rays=d, n=bad.shape[0], k=k)
        assert (words(got) == H.contract_records(bad, max(k, 1))).all(), what
    finally:
        dev.mem.free(d)


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_reference_shaped_kernel(mem, name, grid, compress):
    """"traverse.variant" 1, the kernel of the statistics entry point: records, the eight counters (an inadmissible ray is no ray that hit the grid), the
    per-ray step counts (0 for an inadmissible ray) and, with "traverse.id_is_steps", the step count in Hit.id"""
    from hagrid_amd import api
    w = _world(name, grid, compress)
    dev = Device(mem, w)
    try:
        mem.set_option("traverse.variant", 1)
        api.setup_traversal(dev.grid)
        w.check(dev.run(), "variant 1")
        d_hits = alloc_out(mem, 16 * w.n); d_steps = alloc_out(mem, 4 * w.n)
        st = api.traverse_grid_stats(dev.grid, dev.d_tris, dev.d_rays, d_hits, w.n, d_steps)
        steps = fetch(mem, d_steps, np.int32, w.n)
        w.check(fetch(mem, d_hits, api.HIT_DTYPE, w.n), "statistics entry point")
        mem.free(d_hits); mem.free(d_steps)
        assert st == w.stats, (st, w.stats)
        assert (steps == w.steps).all() and (steps[w.inadmissible] == 0).all() and steps.max() > 3
        mem.set_option("traverse.id_is_steps", 1)
        stepped = dev.run()
        assert (stepped["id"] == w.steps).all()
        w.check(stepped, "id_is_steps", ids=False)
        mem.set_option("traverse.id_is_steps", 0)
        _only_inadmissible(dev, "variant 1, inadmissible rays only")
    finally:
        mem.set_option("traverse.id_is_steps", 0); mem.set_option("traverse.variant", 0)
        dev.close()


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_v2_kernels(mem, name, grid, compress):
    """the latency-oriented kernel of the construction format, with 32-bit ("traverse.narrow" 1) and 64-bit addressing, with and without ray binning"""
    from hagrid_amd import api
    w = _world(name, grid, compress)
    dev = Device(mem, w)
    try:
        mem.set_option("traverse.variant", 2)
        api.setup_traversal(dev.grid)
        for narrow in (1, 0):
            mem.set_option("traverse.narrow", narrow)
            for binning in (0, 1):
                mem.set_ray_binning(binning)
                w.check(dev.run(), f"v2 narrow={narrow} binning={binning}")
        _only_inadmissible(dev, "v2, inadmissible rays only")
    finally:
        mem.set_ray_binning(0); mem.set_option("traverse.narrow", 1); mem.set_option("traverse.variant", 0)
        dev.close()


@pytest.mark.parametrize("fmt_name", list(IMAGE_FORMATS))
@pytest.mark.parametrize("name", list(image_scenes()))
def test_image_kernels_on_every_format_and_scene(mem, name, fmt_name):
    """the scenes and traversal-image formats of test_image_kernel_gives_the_oracle_hits, each with the catalogue of its own grid: the image kernel without the
    tail mode ("traverse.variant" 4), the default dispatch and v2, the block layouts with and without the table-free one, binned"""
    from hagrid_amd import api
    from oracle import oracle as O
    fmt, slim, general = IMAGE_FORMATS[fmt_name]
    tris, params = image_scenes()[name]
    w = World(tris, O.Grid.full(tris, **params), mesh=False)
    dev = Device(mem, w)
    try:
        mem.set_option("traverse.image", fmt); mem.set_option("traverse.image_slim", slim); mem.set_option("traverse.image_general", general)
        for uniform in ((1, 0) if slim == 1 and general == 1 else (1,)):
            mem.set_option("traverse.image_uniform", uniform)
            for variant in (4, 0, 2):
                mem.set_option("traverse.variant", variant)
                api.setup_traversal(dev.grid)
                w.check(dev.run(), f"uniform={uniform} variant={variant}")
        mem.set_option("traverse.image_uniform", 1)
        mem.set_ray_binning(1); mem.set_option("traverse.variant", 4)
        api.setup_traversal(dev.grid)
        w.check(dev.run(), "variant 4, binned")
    finally:
        mem.set_ray_binning(0); mem.set_option("traverse.variant", 0); mem.set_option("traverse.image", 2); mem.set_option("traverse.image_uniform", 1)
        mem.set_option("traverse.image_slim", 1); mem.set_option("traverse.image_general", 1)
        dev.close()


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_tail_kernel_settings(mem, name, grid, compress):
    """traverse_kernel_tail: with and without the tail mode, no / all tiles starting with four lanes per ray, one and two ids per round, the head share; the
    rays as an unordered batch and -- "traverse.image_width" -- inside tile packets, where a second launch over the same buffer follows the tile order the
    first one learned; ray binning off, on and automatic"""
    from hagrid_amd import api
    w = _world(name, grid, compress)
    dev = Device(mem, w)
    try:
        api.setup_traversal(dev.grid)
        for tail, quad, dual, head in ((1, -1, -1, 20), (0, 0, -1, 20), (1, 0, 0, 20), (1, 0, 1, 20), (1, 100, 0, 20), (1, 100, 1, 11), (1, 30, 1, 0)):
            mem.set_option("traverse.tail", tail); mem.set_option("traverse.quad_tail", quad); mem.set_option("traverse.tail_dual", dual)
            mem.set_option("traverse.quad_head", head)
            for width in (0, 64, 200):
                mem.set_option("traverse.image_width", width)
                for binning in ((0, 1, 2) if width == 0 else (0,)):
                    mem.set_ray_binning(binning)
                    for launch in range(3 if width else 1):          # (the same buffer again: the order the launch before left is followed)
                        w.check(dev.run(), f"tail={tail} quad_tail={quad} dual={dual} head={head} width={width} binning={binning} launch={launch}")
        mem.set_option("traverse.image_width", 0)
        _only_inadmissible(dev, "default dispatch, inadmissible rays only")
    finally:
        mem.set_ray_binning(0); mem.set_option("traverse.image_width", 0)
        mem.set_option("traverse.tail", 1); mem.set_option("traverse.quad_tail", -1); mem.set_option("traverse.tail_dual", -1); mem.set_option("traverse.quad_head", 20)
        dev.close()


@pytest.mark.parametrize("name,grid,compress", DEFAULT_CASES, ids=DEFAULT_IDS)
def test_any_hit_and_barycentrics(mem, name, grid, compress):
    """HAGRID_TRAVERSE_ANY_HIT and HAGRID_TRAVERSE_UVS against traverse_ex of the oracle: the default dispatch, binned, and v2.  An inadmissible ray keeps the
    contract's record under every flag; the -0 family gets the +0 family's barycentrics."""
    from hagrid_amd import api
    from oracle import oracle as O
    w = _world(name, grid, compress)
    dev = Device(mem, w)
    try:
        api.setup_traversal(dev.grid)
        for binning, variant in ((0, 0), (1, 0), (0, 2)):
            mem.set_ray_binning(binning); mem.set_option("traverse.variant", variant)
            for flags, oflags in ((api.UVS, O.UVS), (api.ANY_HIT, O.ANY_HIT), (api.ANY_HIT | api.UVS, O.ANY_HIT | O.UVS)):
                want = w.G.traverse_ex(w.tris, w.rays, oflags, nthreads=8)
                got = dev.run(flags)
                what = f"flags={flags} binning={binning} variant={variant}"
                assert (words(got) == words(want)).all(), what
                assert (words(got[w.inadmissible]) == H.contract_records(w.rays[w.inadmissible])).all(), what
                c = got[w.pos]
                assert (words(c[w.fam == "a"]) == words(c[w.fam == "b"])).all(), what
                if not flags & api.ANY_HIT:
                    w.check(got, what, uvs=want)
    finally:
        mem.set_ray_binning(0); mem.set_option("traverse.variant", 0)
        dev.close()


@pytest.mark.parametrize("name,grid,compress", DEFAULT_CASES, ids=DEFAULT_IDS)
def test_multi_hit(mem, name, grid, compress, tmp_path):
    """the k nearest hits, k = 1, 2, 8, against the host walk tests/cpp/multi_hit_host.cpp over the same grid arrays: every record bit for bit; an inadmissible
    ray gets k times the contract's record; k = 1 is the nearest-hit record wherever that one is the brute force's"""
    w = _world(name, grid, compress)
    dev = Device(mem, w)
    exe = M.build_host(tmp_path)
    arrays = M.oracle_grid_arrays(w.G)
    try:
        for k in (1, 2, 8):
            got = dev.run(k=k)
            want = M.host_walk(exe, tmp_path, arrays, w.tris, w.rays, k)
            assert (words(got) == words(want)).all(), k
            rec = words(got).reshape(w.n, k, 4)
            assert (rec[w.inadmissible].reshape(-1, 4) == H.contract_records(w.rays[w.inadmissible], k)).all(), k
            c = rec[w.pos]
            assert (c[w.fam == "a"] == c[w.fam == "b"]).all(), k
            if k == 1:
                general = np.isin(w.fam, list("abcdefgh"))
                assert (c[general][:, 0, 0:2] == words(w.fixture[general])[:, 0:2]).all()
        _only_inadmissible(dev, "multi-hit, inadmissible rays only", k=8)
    finally:
        dev.close()


@pytest.fixture(scope="module")
def multi_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("multi_hit_host")
    return M.build_host(d), d


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_skew_rays_next_to_voxel_planes(mem, name, grid, compress, multi_host):
    """H.skew_rays, the admissible rays whose walk converts values beyond the range of int ("What remains"): every kernel gives the records of
    the oracle with the device's conversions (ORC_WALK_DEVICE_F2I) -- which are the brute force's, bit for bit -- embedded among ordinary rays; the multi-hit
    kernel gives the lists of the host walk (the same include/hagrid/cell_walk.h, the conversion written out), every record bit for bit"""
    from hagrid_amd import api
    from oracle import oracle as O
    tris = H.make_tris(name)
    G = H.oracle_grid(tris, H.GRID_PARAMS[grid], compress)
    skew = H.skew_rays(tris, G)
    rays, pos = H.embed(skew, G.bbox_min, G.bbox_max, seed=3)
    O.walk_capped()
    with O.walk_mode(O.DEVICE_F2I):
        want, _ = G.traverse(tris, rays, nthreads=8)
    assert O.walk_capped() == (0, -1)
    bf = O.brute_force(tris, skew, nthreads=8)
    assert (words(want[pos])[:, 0:2] == words(bf)[:, 0:2]).all()
    w = World.__new__(World)
    w.tris, w.G, w.rays, w.n = tris, G, rays, rays.shape[0]
    dev = Device(mem, w)
    try:
        for variant, image_width in ((1, 0), (2, 0), (4, 0), (0, 0), (0, 64)):
            mem.set_option("traverse.variant", variant); mem.set_option("traverse.image_width", image_width)
            api.setup_traversal(dev.grid)
            for launch in range(2 if image_width else 1):
                got = dev.run()
                bad = (words(got) != words(want)).any(axis=1)
                assert not bad.any(), (variant, image_width, launch, int(bad.sum()), np.flatnonzero(bad)[:5], got[bad][:2], want[bad][:2])
        exe, d = multi_host
        arrays = M.oracle_grid_arrays(G)
        for k in (1, 2, 8):
            got = dev.run(k=k)
            lists = M.host_walk(exe, d, arrays, tris, rays, k)
            assert (words(got) == words(lists)).all(), k
            assert (words(got.reshape(w.n, k)[:, 0])[:, 0:2] == words(want)[:, 0:2]).all(), k
    finally:
        mem.set_option("traverse.variant", 0); mem.set_option("traverse.image_width", 0)
        dev.close()
