"""Every allocation-failure exit on the GPU: for each entry point that can answer HAGRID_ENOMEM the sweep runs it once clean in a fresh context, reads how many
allocation requests R it made, and runs it again R times from the same starting state with the i-th request made to fail ("mem.fail_request" of the test library,
host side only).  After every injected run: HAGRID_ENOMEM with a message of its own -- or, at exactly the optional sites of tests/_alloc_failures.py, HAGRID_OK with
the oracle's output --, the descriptor in the state include/hagrid_amd.h promises, the pool's books as they were, a stream without an error, compared outputs
untouched, and a context that builds the oracle's grid and finds the oracle's hits afterwards.  The retry of hagrid_mem_alloc ("give back every cached buffer and
retry once", "mem.fail_malloc") and its re-grow branch are taken on purpose.  Each sweep prints its R and the indices that degraded.

The injection is host side and provokes no fault, but a wrong exit could launch with the pointer that was refused: every exit of the table was read for that before
the sweeps ran on a device, and a site added to the table is to be read the same way.  A sweep stops at the first return that is neither OK nor HAGRID_ENOMEM; HAGRID_EHIP from any call ends the pytest session: nothing more is started on that card."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import _alloc_failures as A
import _poison as P
from _alloc_failures import EHIP, EINVAL, ENOMEM, OK
from _traverse_formats import IMAGE_FORMATS, image_scenes
from hagrid_amd import scene
from test_build_gpu import assert_same_grid

pytestmark = pytest.mark.gpu

STAGES = ("build_grid", "merge_grid", "flatten_grid", "expand_grid", "compress_grid")
NUM_RAYS = 4096
vp = C.c_void_p


# ---- the oracle's side, computed once ---------------------------------------------------------------------------------------------------------

class Reference:
    """the fixture scene, its quarter and its fourfold, and the oracle's grid behind every pass (each its own object: the oracle's passes work in place)"""

    def __init__(self):
        from oracle import oracle as O
        self.O = O
        self.tris = A.fixture_scene()
        self.quarter = A.fixture_scene(750, 32)
        self.fourfold = A.fixture_scene(12000, 33)
        self._stage = {}
        self._built = {}
        self.rays = scene.make_rays_incoherent(*scene.tris_bbox(self.tris), NUM_RAYS, 77)
        self.rays_binned = scene.make_rays_incoherent(*scene.tris_bbox(self.tris), 2 * NUM_RAYS, 78)      # (binning starts above 4096 rays)
        self.rays_image = scene.make_rays_primary(*scene.tris_bbox(self.tris), 128, 64)
        self.rays_big = scene.make_rays_incoherent(*scene.tris_bbox(self.tris), 1 << 18, 80)       # (ray_order.hip: the origin criterion runs from 2^18 rays on)
        self.rays_image_big = scene.make_rays_primary(*scene.tris_bbox(self.tris), 512, 512)
        self._hits = {}

    def built(self, which: str):
        if which not in self._built:
            self._built[which] = self.O.Grid.build(getattr(self, which), A.TOP_DENSITY, A.SND_DENSITY)
        return self._built[which]

    def after(self, stage: str, iters: int = A.EXPAND_ITERS, subset_only: bool = True):
        """the oracle's grid of the fixture scene behind `stage` (None: before build_grid)"""
        key = (stage, iters, subset_only) if stage in ("expand_grid", "compress_grid") else (stage,)
        if key not in self._stage:
            G = self.O.Grid.build(self.tris, A.TOP_DENSITY, A.SND_DENSITY)
            for s in STAGES[1:STAGES.index(stage) + 1]:
                if s == "merge_grid": G.merge(A.ALPHA)
                elif s == "flatten_grid": G.flatten()
                elif s == "expand_grid": G.expand(self.tris, iters, subset_only=subset_only)
                else: assert G.compress()
            self._stage[key] = G
        return self._stage[key]

    def hits(self, name: str, rays, compressed: bool = False):
        key = (name, compressed)
        if key not in self._hits:
            G = self.after("compress_grid" if compressed else "expand_grid")
            self._hits[key] = G.traverse(self.tris, rays, nthreads=4)[0]
        return self._hits[key]


@pytest.fixture(scope="module")
def ref():
    return Reference()


def test_the_fixture_scene_is_on_the_paths(ref):
    """what puts the sweeps on the exits behind queued kernels, stated on the oracle and the build counts: at least three levels, a primitive on the cooperative
    list, a merge of at least five passes that enters the in-place mode"""
    import _fallbacks as F
    from hagrid_amd import api
    G = ref.built("tris")
    assert G.shift + 1 >= 3, G.summary()
    assert F.large_primitives(ref.tris, G.dims, G.bbox_min, G.bbox_max) >= 1
    mem = api.MemManager(keep=True)
    try:
        d_tris = mem.upload(ref.tris)
        grid = api.Grid()
        api.build_grid(mem, d_tris, ref.tris.shape[0], grid, A.TOP_DENSITY, A.SND_DENSITY)
        api.merge_grid(mem, grid, A.ALPHA)
        bc = mem.build_counts()
        assert bc["num_levels"] >= 3 and bc["merge_passes"] >= 5, bc
        assert A.entered_in_place(bc["merge_cells"], bc["merged_cells"], A.ALPHA), (bc["merge_cells"], bc["merged_cells"])
    finally:
        mem.close()


# ---- one context, one run ---------------------------------------------------------------------------------------------------------------------

SCAN_PROBE = 1 << 20
Result = collections.namedtuple("Result", "requests outcome scans two_layouts", defaults=(False,))      # of one run; scans: counted in a clean run, else None


def arm(mem, i):
    """i: 0 (a clean run: the scans are counted), n (the n-th request fails) or ("scan", n) (the n-th look-back scan finds no status words)"""
    if i == 0:
        mem.set_option("mem.fail_scan", SCAN_PROBE)
    elif isinstance(i, tuple):
        mem.set_option("mem.fail_scan", i[1])
    else:
        mem.set_option("mem.fail_request", i)


def disarm(mem, i):
    """behind the call under test: the setting read back 0 shows that it fired; a clean run returns its number of look-back scans"""
    pending = mem.mem_pending()
    if i == 0:
        mem.set_option("mem.fail_scan", 0)
        return SCAN_PROBE - pending[2]
    A.check_fired(pending[2] if isinstance(i, tuple) else pending[0])
    return None


def sweep(entry, what, run, cfg=lambda first: {}):
    """run(i) -> Result: once clean, once per request, once per look-back scan; the outcomes against the table"""
    first = run(0)
    R, S = first.requests, first.scans
    ok = [i for i in range(1, R + 1) if run(i).outcome == "ok"]
    ok_scans = [j for j in range(1, S + 1) if run(("scan", j)).outcome == "ok"]
    print(f"\nalloc-failure sweep {entry} {what}: R = {R}, degraded instead of failing: {sorted(ok)}; look-back scans S = {S}, each refused in turn: {S - len(ok_scans)} failed")
    A.check_outcomes(entry, R, ok, A.optional_indices(entry, R, **cfg(first)), what)
    assert ok_scans == [], f"{entry} {what}: a scan without status words came back OK at scans {ok_scans}"


def guard(rc, what):
    """HAGRID_EHIP ends the session: the card may have faulted, nothing more is started on it"""
    if rc == EHIP:
        pytest.exit(f"{what} answered HAGRID_EHIP: the session ends here, nothing more runs on this card", returncode=3)
    return rc


class Ctx:
    """a fresh context with the fixture's triangles uploaded, a harmless HAGRID_EINVAL provoked (its text must not survive a later failure) and the books taken"""

    def __init__(self, ref, keep, extra=()):
        from hagrid_amd import api
        self.api, self.ref = api, ref
        self.mem = api.MemManager(keep=keep)
        self.keep = keep
        self.L, self.ctx = self.mem._L, self.mem._ctx
        self.d = {name: self.mem.upload(getattr(ref, name)) for name in ("tris",) + tuple(extra)}
        self.d_tris, self.n = self.d["tris"], ref.tris.shape[0]
        g = api.Grid()
        assert self.L.hagrid_build_grid(self.ctx, None, 0, C.byref(g.pod), A.TOP_DENSITY, A.SND_DENSITY) == EINVAL
        self.earlier = self.error()
        assert "no triangles" in self.earlier
        self.base, self.base_usage = self.mem.mem_state(), self.mem.usage()

    def error(self) -> str:
        return (self.L.hagrid_last_error(self.ctx) or b"").decode()

    def close(self):
        self.mem.close()

    # the construction passes through the raw ABI (the return code is the result)
    def call_stage(self, stage, grid, which="tris", iters=A.EXPAND_ITERS):
        L, ctx, pod = self.L, self.ctx, C.byref(grid.pod)
        grid.mem = self.mem
        if stage == "build_grid": return L.hagrid_build_grid(ctx, vp(self.d[which]), getattr(self.ref, which).shape[0], pod, A.TOP_DENSITY, A.SND_DENSITY)
        if stage == "merge_grid": return L.hagrid_merge_grid(ctx, pod, A.ALPHA)
        if stage == "flatten_grid": return L.hagrid_flatten_grid(ctx, pod)
        if stage == "expand_grid": return L.hagrid_expand_grid(ctx, pod, vp(self.d_tris), iters)
        return L.hagrid_compress_grid(ctx, pod)

    def grid_before(self, stage, iters=A.EXPAND_ITERS):
        """a grid of the fixture scene with every pass before `stage` run"""
        grid = self.api.Grid()
        for s in STAGES[:STAGES.index(stage)]:
            rc = guard(self.call_stage(s, grid, iters=iters), s)
            assert rc >= 0, (s, rc, self.error())
        return grid

    def full_grid(self, compress=False):
        return self.grid_before("compress_grid") if not compress else self.finish(self.grid_before("compress_grid"), "expand_grid", compress=True)

    def finish(self, grid, stage, compress=False):
        """the passes behind `stage`"""
        for s in STAGES[STAGES.index(stage) + 1:]:
            if s == "compress_grid" and not compress:
                break
            rc = guard(self.call_stage(s, grid), s)
            assert rc >= 0, (s, rc, self.error())
        return grid

    def requests(self) -> int:
        return self.mem.mem_state()["requests"]

    def inject(self, i):
        arm(self.mem, i)

    def fired(self, i):
        return disarm(self.mem, i)

    def synchronize_ok(self):
        rc = guard(self.L.hagrid_ctx_synchronize(self.ctx), "hagrid_ctx_synchronize")
        assert rc == OK, (rc, self.error())

    def books_back_to_base(self, what):
        """after the test has freed what the descriptors still named"""
        A.check_books(self.base, self.mem.mem_state(), what=what)
        if not self.keep:
            A.check_usage(self.base_usage, self.mem.usage(), what)

    def hits_of(self, grid, rays, setup=True):
        """hits of a launch into a poisoned buffer"""
        mem = self.mem
        d_rays = mem.upload(rays); d_hits = P.alloc_out(mem, 16 * rays.shape[0])
        if setup:
            self.api.setup_traversal(grid)
        self.api.traverse_grid(grid, self.d_tris, d_rays, d_hits, rays.shape[0])
        hits = P.fetch(mem, d_hits, self.api.HIT_DTYPE, rays.shape[0]).copy()
        mem.free(d_rays); mem.free(d_hits)
        return hits

    def works_afterwards(self, stage="build_grid", iters=A.EXPAND_ITERS, subset_only=True):
        """the same pass from a fresh build in the SAME context, without injection, gives the oracle's arrays; behind the last pass 4096 incoherent rays find the
        oracle's hits"""
        grid = self.grid_before(stage, iters=iters)
        rc = guard(self.call_stage(stage, grid, iters=iters), stage)
        assert rc >= 0, (stage, rc, self.error())
        assert_same_grid(grid.download(), self.ref.after(stage, iters, subset_only), (stage, "again, no injection"))
        compressed = stage == "compress_grid"
        if not compressed:
            grid.free()
            grid = self.full_grid()
        same_hits(self.hits_of(grid, self.ref.rays), self.ref.hits("incoherent", self.ref.rays, compressed), (stage, "hits afterwards"))
        grid.free()


def same_hits(got, want, what):
    assert (got["id"] == want["id"]).all() and (got["t"].view(np.uint32) == want["t"].view(np.uint32)).all(), what
    assert (got["u"] == 0).all() and (got["v"] == 0).all(), what


def pod_bytes(grid) -> bytes:
    return bytes(memoryview(grid.pod).cast("B"))


# ---- the construction passes --------------------------------------------------------------------------------------------------------------------

BUILD_STATES = {"first": None, "second": "tris", "quarter_after": "quarter", "fourfold_after": "fourfold"}


def run_build(ref, keep, state, i):
    """build_grid in one of the four pool states, its i-th request failing (0: none).  Returns (requests made, 'ok' | 'enomem')."""
    which = BUILD_STATES[state] or "tris"
    c = Ctx(ref, keep, extra=("quarter", "fourfold"))
    try:
        if BUILD_STATES[state]:                                # a construction of the fixture scene before it: the arena's hint
            g0 = c.api.Grid()
            assert guard(c.call_stage("build_grid", g0), "build_grid") == OK
            g0.free()
        grid = c.api.Grid()
        C.memset(C.addressof(grid.pod), 0xA5, C.sizeof(grid.pod))       # "byte-equal to what it was before the call"
        pod0, before, usage0, r0 = pod_bytes(grid), c.mem.mem_state(), c.mem.usage(), c.requests()
        c.inject(i)
        rc = guard(c.call_stage("build_grid", grid, which), "build_grid")
        made = c.requests() - r0
        assert rc in (OK, ENOMEM), (rc, c.error())
        scans = c.fired(i)
        if rc == ENOMEM:
            assert i, "build_grid without injection answered HAGRID_ENOMEM"
            A.check_error_text(rc, c.error(), c.earlier)
            A.check_descriptor_unchanged(pod0, pod_bytes(grid), f"build_grid {state} request {i}")
            A.check_books(before, c.mem.mem_state(), what=f"build_grid {state} request {i}")
            if not keep:
                A.check_usage(usage0, c.mem.usage(), f"build_grid {state} request {i}")
        else:
            assert_same_grid(grid.download(), ref.built(which), ("build_grid", state, i))
            grid.free()
        c.synchronize_ok()
        c.books_back_to_base(f"build_grid {state} request {i}")
        if i:
            c.works_afterwards("build_grid")
        return Result(made, "ok" if rc == OK else "enomem", scans)
    finally:
        c.close()


@pytest.mark.parametrize("keep", [False, True], ids=["release", "keep"])
@pytest.mark.parametrize("state", list(BUILD_STATES))
def test_build_grid_sweep(ref, state, keep):
    sweep("build_grid", f"{state} keep={keep}", lambda i: run_build(ref, keep, state, i), lambda first: dict(later_build=BUILD_STATES[state] is not None))


PASS_CONFIGS = {
    "merge_grid": [("defaults", {}, {}), ("wide_cells", {"merge.narrow_cells": 0}, {})],
    "flatten_grid": [("defaults", {}, {})],
    "expand_grid": [(f"subset{s}_iters{k}", {"expand.subset_only": s}, {"iters": k}) for s in (1, 0) for k in (1, 3)],
    "compress_grid": [("defaults", {}, {})],
}


def run_pass(ref, keep, stage, options, cfg, i):
    iters = cfg.get("iters", A.EXPAND_ITERS)
    subset_only = bool(options.get("expand.subset_only", 1))
    spec = A.ENTRY_POINTS[stage]
    what = f"{stage} {options} {cfg} request {i}"
    c = Ctx(ref, keep)
    try:
        for k, v in options.items():
            c.mem.set_option(k, v)
        grid = c.grid_before(stage, iters=iters)
        prior = ref.after(STAGES[STAGES.index(stage) - 1], iters, subset_only)
        pod0, before, r0 = pod_bytes(grid), c.mem.mem_state(), c.requests()
        c.inject(i)
        rc = guard(c.call_stage(stage, grid, iters=iters), stage)
        made = c.requests() - r0
        assert rc in (OK, 1, ENOMEM), (rc, c.error())
        scans = c.fired(i)
        if rc == ENOMEM:
            assert i, f"{stage} without injection answered HAGRID_ENOMEM"
            A.check_error_text(rc, c.error(), c.earlier)
            if spec["state"] == "released":
                A.check_released(grid.cells, grid.ref_ids, grid.num_cells, grid.num_refs, grid.entries, what)
                A.check_books(before, c.mem.mem_state(), released_slots=2, released_bytes=None, what=what)      # (the two slots' sizes: the pool's choice)
                assert c.L.hagrid_mem_free(c.ctx, vp(grid.entries)) == OK, "entries are the caller's to free"       # exactly once: a second free is an error
                assert c.L.hagrid_mem_free(c.ctx, vp(grid.entries)) == EINVAL
                grid.pod.entries = None
            else:
                A.check_descriptor_unchanged(pod0, pod_bytes(grid), what)
                A.check_books(before, c.mem.mem_state(), what=what)
                assert_same_grid(grid.download(), prior, (what, "unchanged"))
                grid.free()
        else:
            if stage == "compress_grid":
                assert rc == 1
            assert_same_grid(grid.download(), ref.after(stage, iters, subset_only), (what, "degraded" if i else "clean"))
            grid.free()
        c.synchronize_ok()
        c.books_back_to_base(what)
        if i:
            c.works_afterwards(stage, iters, subset_only)
        return Result(made, "enomem" if rc == ENOMEM else "ok", scans)
    finally:
        c.close()


def r256(n: int) -> int:
    return (max(int(n), 4) + 255) & ~255


@pytest.mark.parametrize("keep", [False, True], ids=["release", "keep"])
@pytest.mark.parametrize("stage,name,options,cfg", [(s, n, o, k) for s, cs in PASS_CONFIGS.items() for n, o, k in cs], ids=lambda v: v if isinstance(v, str) else "")
def test_construction_pass_sweep(ref, stage, name, options, cfg, keep):
    sweep(stage, f"{name} keep={keep}", lambda i: run_pass(ref, keep, stage, options, cfg, i), lambda first: cfg)


# ---- setup_traversal, once per image format ---------------------------------------------------------------------------------------------------------

# ... and the default options on a grid whose uniform layout gets the compact layout built next to it: the optional site of trav_image.hip build_blocks
FORMATS = dict(IMAGE_FORMATS, flat_two_layouts=IMAGE_FORMATS["flat"])


def format_matches(key, fmt) -> bool:
    """the layout a format of IMAGE_FORMATS stands for: a block layout (26-bit ids where asked for), or the general one"""
    if not fmt:
        return False
    if key == "flat_two_layouts":
        return fmt["two_layouts"]
    if key == "flat_general":
        return fmt["general"]
    return not fmt["general"] and (key != "flat_slim26" or fmt["slim_id_bits"] == 26)


def set_format(mem, key):
    image, slim, general = FORMATS[key]
    mem.set_option("traverse.image", image); mem.set_option("traverse.image_slim", slim); mem.set_option("traverse.image_general", general)


@pytest.fixture(scope="module")
def format_scenes():
    """{format: (scene name, tris, build arguments, the oracle's grid, rays, the oracle's hits)}: the smallest scene of image_scenes() that gives the layout"""
    from hagrid_amd import api
    from oracle import oracle as O
    scenes = sorted(image_scenes().items(), key=lambda kv: kv[1][0].shape[0])
    chosen = {}
    mem = api.MemManager(keep=True)
    try:
        for name, (tris, kw) in scenes:
            if len(chosen) == len(FORMATS):
                break
            tris = np.ascontiguousarray(tris, dtype=np.float32)
            d_tris = mem.upload(tris)
            grid = api.build_all(mem, d_tris, tris.shape[0], **kw)
            for key in FORMATS:
                if key in chosen:
                    continue
                set_format(mem, key)
                api.setup_traversal(grid)
                if format_matches(key, mem.image_format(grid)):
                    chosen[key] = (name, tris, kw)
            grid.free(); mem.free(d_tris)
    finally:
        mem.close()
    assert sorted(chosen) == sorted(FORMATS), f"no scene of image_scenes() gives the layouts {sorted(set(FORMATS) - set(chosen))}"
    out, oracle = {}, {}
    for key, (name, tris, kw) in chosen.items():
        if name not in oracle:
            G = O.Grid.full(tris, **kw)
            rays = scene.make_rays_incoherent(G.bbox_min, G.bbox_max, NUM_RAYS, 79)
            oracle[name] = (G, rays, G.traverse(tris, rays, nthreads=4)[0])
        out[key] = (name, tris, kw) + oracle[name]
    return out


def run_setup(key, case, i):
    from hagrid_amd import api
    name, tris, kw, G, rays, want = case
    what = f"setup_traversal {key} on {name} request {i}"
    mem = api.MemManager(keep=True)
    L, ctx = mem._L, mem._ctx
    try:
        d_tris = mem.upload(tris); d_rays = mem.upload(rays); d_hits = P.alloc_out(mem, 16 * NUM_RAYS)
        assert L.hagrid_build_grid(ctx, None, 0, C.byref(api.Grid().pod), 0.12, 2.4) == EINVAL
        earlier = L.hagrid_last_error(ctx).decode()
        base = mem.mem_state()
        grid = api.build_all(mem, d_tris, tris.shape[0], **kw)
        set_format(mem, key)

        def launch(tag):
            P.poison(mem, d_hits, 16 * NUM_RAYS)
            api.traverse_grid(grid, d_tris, d_rays, d_hits, NUM_RAYS)
            same_hits(P.fetch(mem, d_hits, api.HIT_DTYPE, NUM_RAYS), want, (what, tag))

        pod0, before, r0 = pod_bytes(grid), mem.mem_state(), mem.mem_state()["requests"]
        arm(mem, i)
        rc = guard(L.hagrid_setup_traversal(ctx, C.byref(grid.pod)), "hagrid_setup_traversal")
        made = mem.mem_state()["requests"] - r0
        text = L.hagrid_last_error(ctx).decode()                # (before image_format asks for an image that may not be there: that is an error of its own)
        assert rc in (OK, ENOMEM), (rc, text)
        scans = disarm(mem, i)
        fmt = mem.image_format(grid)
        A.check_descriptor_unchanged(pod0, pod_bytes(grid), what)
        if rc == ENOMEM:
            assert i
            A.check_error_text(rc, text, earlier)
            assert fmt == {}, f"{what}: a traversal image is left behind a setup that failed: {fmt}"
            A.check_books(before, mem.mem_state(), what=what)
            assert_same_grid(grid.download(), G, (what, "unchanged"))
            launch("construction format behind the failure")
            api.setup_traversal(grid)                           # the context works afterwards: the image is built, the hits are the oracle's
            assert format_matches(key, mem.image_format(grid)), what
        elif i and key == "flat_two_layouts":                  # degraded: the second table is not built, the uniform layout serves every batch
            assert fmt and fmt["uniform"] and not fmt["two_layouts"], (what, fmt)
        else:
            assert format_matches(key, fmt), (what, fmt)
        launch("with the image")
        assert guard(L.hagrid_ctx_synchronize(ctx), "hagrid_ctx_synchronize") == OK
        grid.free()                                             # (takes the image with it)
        A.check_books(base, mem.mem_state(), what=what)
        return Result(made, "enomem" if rc == ENOMEM else "ok", scans, bool(fmt.get("two_layouts")))
    finally:
        mem.close()


@pytest.mark.parametrize("key", list(FORMATS))
def test_setup_traversal_sweep(format_scenes, key):
    case = format_scenes[key]
    sweep("setup_traversal", f"{key} on {case[0]}", lambda i: run_setup(key, case, i), lambda first: dict(two_layouts=first.two_layouts))


# ---- launches over the finished grid (keep contexts) ---------------------------------------------------------------------------------------------

class Launches(Ctx):
    """a keep context with the finished grid of the fixture scene, its traversal image, and what a launch needs"""

    def __init__(self, ref, rays):
        super().__init__(ref, True)
        self.rays = rays
        self.nr = rays.shape[0]
        self.d_rays = self.mem.upload(rays)
        self.d_hits = P.alloc_out(self.mem, 16 * self.nr)
        self.base = self.mem.mem_state()
        self.grid = self.full_grid()
        self.api.setup_traversal(self.grid)
        self.pod0 = pod_bytes(self.grid)

    def raw_hits(self):
        return P.fetch(self.mem, self.d_hits, np.uint8, 16 * self.nr)

    def end(self, what):
        self.synchronize_ok()
        A.check_descriptor_unchanged(self.pod0, pod_bytes(self.grid), what)
        self.grid.free()
        A.check_books(self.base, self.mem.mem_state(), what=what)


def run_traverse_binned(ref, i, mode=1):
    """mode 1: binning forced, 8192 rays.  mode 2: automatic, 2^18 rays -- the words of the automatic mode (a hard failure) and, from that many rays on, the row
    scores of the origin criterion (optional: the first criterion stands alone) are requested behind the four binning buffers"""
    rays = ref.rays_binned if mode == 1 else ref.rays_big
    want = ref.hits(f"binned{mode}", rays)
    c = Launches(ref, rays)
    what = f"traverse_grid, binning mode {mode}, request {i}"
    try:
        c.mem.set_ray_binning(mode)
        before, r0 = c.mem.mem_state(), c.requests()
        c.inject(i)
        rc = guard(c.L.hagrid_traverse_grid(c.ctx, C.byref(c.grid.pod), vp(c.d_tris), vp(c.d_rays), vp(c.d_hits), c.nr), "hagrid_traverse_grid")
        made = c.requests() - r0
        assert rc in (OK, ENOMEM), (rc, c.error())
        scans = c.fired(i)
        c.synchronize_ok()
        if rc == ENOMEM:
            assert i
            A.check_error_text(rc, c.error(), c.earlier)
            A.check_untouched(c.raw_hits(), what)
            A.check_books(before, c.mem.mem_state(), what=what)
            c.api.traverse_grid(c.grid, c.d_tris, c.d_rays, c.d_hits, c.nr)          # the context works afterwards: the same launch, binned
        elif i:
            assert c.error() == c.earlier, f"{what}: an optional buffer's failure left a message: {c.error()!r}"
        same_hits(P.fetch(c.mem, c.d_hits, c.api.HIT_DTYPE, c.nr), want, what)
        A.check_books(before, c.mem.mem_state(), what=what)
        c.end(what)
        return Result(made, "enomem" if rc == ENOMEM else "ok", scans)
    finally:
        c.close()


def test_traverse_grid_with_ray_binning_sweep(ref):
    sweep("traverse_grid_binned", "ray binning forced", lambda i: run_traverse_binned(ref, i))


def test_traverse_grid_with_automatic_binning_sweep(ref):
    sweep("traverse_grid_auto_binned", "automatic binning, 2^18 rays", lambda i: run_traverse_binned(ref, i, mode=2))


def run_traverse_tile_order(ref, i, width=128):
    """two launches over one buffer of rays in image order.  "traverse.image_width" = 128, 8192 rays: the tile-order buffer of the buffer's hint slot is taken.
    "traverse.image_width" = 0 (the row length is looked for on the device), 512 x 512 rays: from 2^18 rays on the origin criterion takes the row scores, and
    the second launch, which knows the rows, the tile-order buffer"""
    rays = ref.rays_image if width else ref.rays_image_big
    want = ref.hits(f"image{width}", rays)
    c = Launches(ref, rays)
    what = f"traverse_grid, traverse.image_width {width}, request {i}"
    try:
        c.mem.set_option("traverse.image_width", width)
        before, r0 = c.mem.mem_state(), c.requests()
        c.inject(i)
        for launch in (1, 2):
            rc = guard(c.L.hagrid_traverse_grid(c.ctx, C.byref(c.grid.pod), vp(c.d_tris), vp(c.d_rays), vp(c.d_hits), c.nr), "hagrid_traverse_grid")
            assert rc == OK, (what, launch, rc, c.error())              # every request of an un-binned launch is optional
            same_hits(P.fetch(c.mem, c.d_hits, c.api.HIT_DTYPE, c.nr), want, (what, launch))
            P.poison(c.mem, c.d_hits, 16 * c.nr)
        made = c.requests() - r0
        scans = c.fired(i)
        if i:
            assert c.error() == c.earlier, f"{what}: an optional buffer's failure left a message: {c.error()!r}"
        A.check_books(before, c.mem.mem_state(), what=what)
        c.api.traverse_grid(c.grid, c.d_tris, c.d_rays, c.d_hits, c.nr)
        same_hits(P.fetch(c.mem, c.d_hits, c.api.HIT_DTYPE, c.nr), want, (what, "afterwards"))
        c.end(what)
        return Result(made, "ok", scans)
    finally:
        c.close()


def test_traverse_grid_tile_order_sweep(ref):
    sweep("traverse_grid_tile_order", "traverse.image_width, two launches", lambda i: run_traverse_tile_order(ref, i))


def test_traverse_grid_row_detection_sweep(ref):
    sweep("traverse_grid_row_detect", "row length looked for, 2^18 rays, two launches", lambda i: run_traverse_tile_order(ref, i, width=0))


def run_stats(ref, i):
    from hagrid_amd.lib import TraversalStats
    want = ref.hits("incoherent", ref.rays)
    c = Launches(ref, ref.rays)
    what = f"traverse_grid_stats request {i}"
    try:
        st = TraversalStats()
        before, r0 = c.mem.mem_state(), c.requests()
        c.inject(i)
        rc = guard(c.L.hagrid_traverse_grid_stats(c.ctx, C.byref(c.grid.pod), vp(c.d_tris), vp(c.d_rays), vp(c.d_hits), c.nr, None, C.byref(st)), "hagrid_traverse_grid_stats")
        made = c.requests() - r0
        assert rc in (OK, ENOMEM), (rc, c.error())
        scans = c.fired(i)
        if rc == ENOMEM:
            A.check_error_text(rc, c.error(), c.earlier)
            A.check_untouched(c.raw_hits(), what)
            assert st.as_dict()["rays"] == 0
            A.check_books(before, c.mem.mem_state(), what=what)
            assert c.api.traverse_grid_stats(c.grid, c.d_tris, c.d_rays, c.d_hits, c.nr)["rays"] == c.nr
        else:
            assert st.as_dict()["rays"] == c.nr
        same_hits(P.fetch(c.mem, c.d_hits, c.api.HIT_DTYPE, c.nr), want, what)
        c.end(what)
        return Result(made, "enomem" if rc == ENOMEM else "ok", scans)
    finally:
        c.close()


def test_traverse_grid_stats_sweep(ref):
    sweep("traverse_grid_stats", "", lambda i: run_stats(ref, i))


@pytest.fixture(scope="module")
def lattice(ref):
    """(origin, size, n, band, the numpy statement's records) of a small lattice over the fixture scene's cluster"""
    origin = np.float32([0.55, 0.55, 0.55]); n = (12, 10, 8)
    size = (np.float32(0.1) / np.float32(n)).astype(np.float32)
    band = 0.02
    return origin, size, n, band, scene.distance_lattice(ref.tris, origin, size, n, band)


def run_distance(ref, lattice, i, with_image):
    import _distance as D
    origin, size, n, band, want = lattice
    voxels = int(np.prod(n))
    c = Launches(ref, ref.rays)
    what = f"distance_lattice (image: {with_image}) request {i}"
    try:
        mem = c.mem
        if not with_image:
            mem.set_option("traverse.image", 0); c.api.setup_traversal(c.grid); mem.set_option("traverse.image", 2)       # (drops the image: the largest id is read back)
        d_ws = mem.alloc(8 * voxels); d_ids = P.alloc_out(mem, 4 * voxels); d_d2 = P.alloc_out(mem, 4 * voxels); d_rec = P.alloc_out(mem, 32 * voxels)
        before, r0 = mem.mem_state(), c.requests()
        c.inject(i)
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
        call = lambda: c.L.hagrid_distance_lattice(c.ctx, C.byref(c.grid.pod), vp(c.d_tris), f3(origin), f3(size), (C.c_int * 3)(*n), C.c_float(band), vp(d_ws), vp(d_ids), vp(d_d2),
                                                   vp(d_rec), None, 0)
        rc = guard(call(), "hagrid_distance_lattice")
        made = c.requests() - r0
        assert rc in (OK, ENOMEM), (rc, c.error())
        scans = c.fired(i)
        c.synchronize_ok()
        if rc == ENOMEM:
            A.check_error_text(rc, c.error(), c.earlier)
            for d, b in ((d_ids, 4), (d_d2, 4), (d_rec, 32)):
                A.check_untouched(P.fetch(mem, d, np.uint8, b * voxels), what)
            A.check_books(before, mem.mem_state(), what=what)
            assert guard(call(), "hagrid_distance_lattice") == OK
        got_ids = P.fetch(mem, d_ids, np.int32, voxels); got_d2 = P.fetch(mem, d_d2, np.float32, voxels); got_rec = P.fetch(mem, d_rec, scene.CLOSEST_DTYPE, voxels)
        assert (got_ids == want["id"]).all() and (got_d2.view(np.uint32) == want["d2"].view(np.uint32)).all(), what
        D.assert_records_equal(got_rec, want, what)
        assert (want["id"] >= 0).any() and (want["id"] < 0).any()
        for d in (d_ws, d_ids, d_d2, d_rec):
            mem.free(d)
        c.end(what)
        return Result(made, "enomem" if rc == ENOMEM else "ok", scans)
    finally:
        c.close()


@pytest.mark.parametrize("with_image", [True, False], ids=["image", "no_image"])
def test_distance_lattice_sweep(ref, lattice, with_image):
    sweep("distance_lattice", f"image: {with_image}", lambda i: run_distance(ref, lattice, i, with_image))


def run_scene_create(ref, i):
    from hagrid_amd import lib
    c = Ctx(ref, True)
    what = f"scene_create request {i}"
    try:
        mem = c.mem
        verts = np.ascontiguousarray(scene.tri_vertices(ref.tris).reshape(-1, 3), dtype=np.float32)
        want = scene.assemble_tris([(verts, None)])[0]
        d_verts = mem.upload(verts); d_out = P.alloc_out(mem, 48 * c.n)
        mesh = lib.Mesh(); mesh.vertices = d_verts; mesh.num_vertices = verts.shape[0]; mesh.indices = None; mesh.num_tris = c.n; mesh.vertex_stride = 12
        before, r0 = mem.mem_state(), c.requests()
        h = vp(0xdead)
        c.inject(i)
        rc = guard(c.L.hagrid_scene_create(c.ctx, C.byref(mesh), 1, None, 1, C.byref(h)), "hagrid_scene_create")
        made = c.requests() - r0
        assert rc in (OK, ENOMEM), (rc, c.error())
        scans = c.fired(i)
        if rc == ENOMEM:
            A.check_error_text(rc, c.error(), c.earlier)
            assert not h.value, "scene_create failed and left a handle"
            A.check_books(before, mem.mem_state(), what=what)
            assert guard(c.L.hagrid_scene_create(c.ctx, C.byref(mesh), 1, None, 1, C.byref(h)), "hagrid_scene_create") == OK
        r1 = c.requests()
        assert guard(c.L.hagrid_scene_assemble(c.ctx, h, None, vp(d_out), None), "hagrid_scene_assemble") == OK
        assert c.requests() == r1, "hagrid_scene_assemble made an allocation request: it belongs in the sweep"
        got = P.fetch(mem, d_out, np.float32, 12 * c.n).reshape(-1, 12)
        assert got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), what
        c.L.hagrid_scene_destroy(c.ctx, h)
        c.synchronize_ok()
        A.check_books(before, mem.mem_state(), what=what)
        return Result(made, "enomem" if rc == ENOMEM else "ok", scans)
    finally:
        c.close()


def test_scene_create_sweep(ref):
    sweep("scene_create", "", lambda i: run_scene_create(ref, i))


# ---- the grid as one buffer ------------------------------------------------------------------------------------------------------------------------

def run_blob(ref, entry, i, tmp_path):
    """grid_pack / grid_save / grid_load with the i-th request failing; grid_unpack is asserted to make none"""
    c = Launches(ref, ref.rays)
    want_hits = ref.hits("incoherent", ref.rays)
    G = ref.after("expand_grid")
    what = f"{entry} request {i}"
    path = str(tmp_path / f"{entry}_{i if isinstance(i, int) else 's%d' % i[1]}.hgrid").encode()
    try:
        mem, L, ctx = c.mem, c.L, c.ctx
        if entry == "grid_load":
            assert guard(L.hagrid_grid_save(ctx, C.byref(c.grid.pod), vp(c.d_tris), c.n, path), "hagrid_grid_save") == OK
        before, r0 = mem.mem_state(), c.requests()
        blob, nbytes = vp(0xdead), C.c_size_t(12345)
        g2 = c.api.Grid(); g2.mem = mem
        C.memset(C.addressof(g2.pod), 0xA5, C.sizeof(g2.pod))
        pod2 = pod_bytes(g2)
        t2, n2 = vp(0xbeef), C.c_int32(-7)
        c.inject(i)
        if entry == "grid_pack":
            rc = L.hagrid_grid_pack(ctx, C.byref(c.grid.pod), vp(c.d_tris), c.n, C.byref(blob), C.byref(nbytes))
        elif entry == "grid_save":
            rc = L.hagrid_grid_save(ctx, C.byref(c.grid.pod), vp(c.d_tris), c.n, path)
        else:
            rc = L.hagrid_grid_load(ctx, path, C.byref(g2.pod), C.byref(t2), C.byref(n2))
        guard(rc, entry)
        made = c.requests() - r0
        assert rc in (OK, ENOMEM), (rc, c.error())
        scans = c.fired(i)
        if rc == ENOMEM:
            A.check_error_text(rc, c.error(), c.earlier)
            A.check_books(before, mem.mem_state(), what=what)
            if entry == "grid_pack":
                assert not blob.value and nbytes.value == 12345, what
            elif entry == "grid_save":
                assert not os.path.exists(path.decode()), f"{what}: a file was written"
            else:
                A.check_descriptor_unchanged(pod2, pod_bytes(g2), what)
                assert t2.value == 0xbeef and n2.value == -7, what
            # the context works afterwards: the same call without injection
            if entry == "grid_pack":
                assert guard(L.hagrid_grid_pack(ctx, C.byref(c.grid.pod), vp(c.d_tris), c.n, C.byref(blob), C.byref(nbytes)), entry) == OK
            elif entry == "grid_save":
                assert guard(L.hagrid_grid_save(ctx, C.byref(c.grid.pod), vp(c.d_tris), c.n, path), entry) == OK
            else:
                assert guard(L.hagrid_grid_load(ctx, path, C.byref(g2.pod), C.byref(t2), C.byref(n2)), entry) == OK
        if entry == "grid_save":                              # what was written loads as the oracle's grid
            assert guard(L.hagrid_grid_load(ctx, path, C.byref(g2.pod), C.byref(t2), C.byref(n2)), "hagrid_grid_load") == OK
        if entry == "grid_pack":
            r1 = c.requests()
            assert guard(L.hagrid_grid_unpack(ctx, blob, nbytes.value, C.byref(g2.pod), C.byref(t2), C.byref(n2)), "hagrid_grid_unpack") == OK
            assert c.requests() == r1, "hagrid_grid_unpack made an allocation request: it belongs in the sweep"
        assert n2.value == c.n
        assert_same_grid(g2.download(), G, what)
        assert mem.download(t2.value, np.float32, 12 * c.n).tobytes() == ref.tris.tobytes(), what
        d_t2 = c.d_tris
        c.d_tris = t2.value
        same_hits(c.hits_of(g2, ref.rays), want_hits, what)
        c.d_tris = d_t2
        g2.free(); mem.free(t2.value)
        c.end(what)
        return Result(made, "enomem" if rc == ENOMEM else "ok", scans)
    finally:
        c.close()


@pytest.mark.parametrize("entry", ["grid_pack", "grid_save", "grid_load"])
def test_blob_sweep(ref, entry, tmp_path):
    sweep(entry, "", lambda i: run_blob(ref, entry, i, tmp_path))


# ---- the retry of hagrid_mem_alloc -------------------------------------------------------------------------------------------------------------------

def test_mem_alloc_retry_gives_back_every_cached_buffer(ref):
    """"mem.fail_malloc" = 1 in front of a hagrid_mem_alloc that nothing cached fits: the first hipMalloc attempt counts as failed, every cached buffer goes back
    to the device, the second attempt is a real hipMalloc.  At that call the cached bytes drop to 0 and usage equals the bytes in use."""
    c = Ctx(ref, True)
    try:
        mem = c.mem
        c.full_grid().free()                                   # a construction leaves cached free slots
        s0 = mem.mem_state()
        assert s0["bytes_cached"] > 0 and mem.usage() == s0["bytes_in_use"] + s0["bytes_cached"]
        mem.set_option("mem.fail_malloc", 1)
        p = mem.alloc(s0["bytes_cached"] + (64 << 20))         # larger than every cached slot, and no slot is re-grown into it without an attempt
        s1 = mem.mem_state()
        assert mem.mem_pending()[1] == 0, "mem.fail_malloc never fired"
        assert s1["mallocs"] - s0["mallocs"] == 2 and s1["requests"] - s0["requests"] == 1
        assert s1["bytes_cached"] == 0, f"{s1['bytes_cached']} bytes still cached behind the retry"
        t = mem.mem_retry()
        assert t["retries"] == 1 and t["cached_behind"] == 0 and t["usage_minus_in_use_behind"] == 0 and 0 < t["bytes_given_back"] <= s0["bytes_cached"], t
        assert mem.usage() == s1["bytes_in_use"] == s0["bytes_in_use"] + r256(s0["bytes_cached"] + (64 << 20))
        assert c.error() == c.earlier                          # the retry succeeded: no message
        mem.free(p)
        c.works_afterwards("build_grid")
    finally:
        c.close()


def test_mem_alloc_retry_behind_a_regrown_slot(ref):
    """the re-grow branch: a keep context whose ONLY free slot is too small for the request -- the slot is released before the failing attempt, the retry finds
    nothing left to give back and succeeds"""
    c = Ctx(ref, True)
    try:
        mem = c.mem
        small = mem.alloc(1 << 16); mem.free(small)
        s0 = mem.mem_state()
        assert s0["bytes_cached"] == 1 << 16
        mem.set_option("mem.fail_malloc", 1)
        p = mem.alloc(1 << 20)
        s1 = mem.mem_state()
        assert mem.mem_pending()[1] == 0 and s1["mallocs"] - s0["mallocs"] == 2
        assert s1["bytes_cached"] == 0 and mem.usage() == s1["bytes_in_use"] == s0["bytes_in_use"] + (1 << 20)
        t = mem.mem_retry()                                    # (the only cached slot was released before the first attempt: the retry found nothing to give back)
        assert t == {"retries": 1, "bytes_given_back": 0, "cached_behind": 0, "usage_minus_in_use_behind": 0}, t
        mem.one(p, 1 << 20)
        assert (mem.download(p, np.uint8, 1 << 20) == 0xFF).all()          # a live buffer
        mem.free(p)
        c.works_afterwards("build_grid")
    finally:
        c.close()


@pytest.mark.parametrize("entry", list(STAGES) + ["setup_traversal"])
def test_retry_inside_a_pass(ref, entry):
    """"mem.fail_malloc" = 1 in front of each construction pass and of setup_traversal, in a keep context whose pool holds cached free slots that fit none of the
    pass's buffers: the pass's first hipMalloc attempt fails, the retry branch runs INSIDE the pass -- every cached buffer goes back, the second attempt is real --
    and the result is the oracle's.  The grid in front of the pass is the oracle's, uploaded: passes run before it in this context would leave cached slots that
    fit every request, and the pass would make no attempt at all.  What the pool caches when the pass returns is the pass's own temporaries again, so the drop to
    0 and "usage equals the bytes in use" are read from the books the branch itself keeps behind its release (hagrid_kat_mem_retry)."""
    c = Ctx(ref, True)
    try:
        mem = c.mem
        stage = entry if entry in STAGES else None
        if stage == "build_grid":
            grid = c.api.Grid()
        else:
            G = ref.after(STAGES[STAGES.index(stage) - 1] if stage else "expand_grid")
            grid = c.api.Grid.upload(mem, G.entries, G.ref_ids, G.cells, G.small_cells, G.bbox_min, G.bbox_max, G.dims, G.shift, G.offsets)
        in_use = mem.mem_state()
        small = [mem.alloc(64) for _ in range(6)]              # six cached slots of 256 bytes: the first buffer they do not fit re-grows one, the retry gives the others back
        for p in small:
            mem.free(p)
        s0 = mem.mem_state()
        assert s0["bytes_cached"] == 6 * 256 and s0["bytes_in_use"] == in_use["bytes_in_use"]
        t0 = mem.mem_retry()
        mem.set_option("mem.fail_malloc", 1)
        if stage is None:
            rc = guard(c.L.hagrid_setup_traversal(c.ctx, C.byref(grid.pod)), entry)
        else:
            rc = guard(c.call_stage(stage, grid), entry)
        assert rc >= 0, (entry, rc, c.error())
        s1 = mem.mem_state()
        assert mem.mem_pending()[1] == 0, f"{entry}: mem.fail_malloc never fired -- the pass made no hipMalloc attempt"
        print(f"\nretry inside {entry}: hipMalloc attempts {s1['mallocs'] - s0['mallocs']} for {s1['requests'] - s0['requests']} requests, cached before {s0['bytes_cached']}, after {s1['bytes_cached']}")
        assert s1["mallocs"] - s0["mallocs"] >= 2
        assert mem.usage() == s1["bytes_in_use"] + s1["bytes_cached"]
        # the branch's own books (hagrid_kat_mem_retry), taken behind its release and before the second attempt: it ran once inside the pass, gave cached slots
        # back -- what the pass's first small requests and the re-grown slot had not taken of the six --, and left nothing cached: usage was the bytes in use
        t1 = mem.mem_retry()
        given = t1["bytes_given_back"] - t0["bytes_given_back"]
        assert t1["retries"] - t0["retries"] == 1, t1
        assert 256 <= given <= s0["bytes_cached"] - 256 and given % 256 == 0, (given, s0["bytes_cached"])
        assert t1["cached_behind"] == 0 and t1["usage_minus_in_use_behind"] == 0, t1
        assert c.error() == c.earlier, c.error()               # the retry succeeded: no message
        if stage is None:
            assert mem.image_format(grid), "no image behind the retry"
            same_hits(c.hits_of(grid, ref.rays, setup=False), ref.hits("incoherent", ref.rays), entry)
        else:
            assert_same_grid(grid.download(), ref.after(stage), (entry, "behind the retry"))
        grid.free()
        c.synchronize_ok()
        c.books_back_to_base(entry)
        c.works_afterwards("build_grid")
    finally:
        c.close()


def test_the_product_refuses_the_injection_settings(ref):
    c = Ctx(ref, True)
    try:
        for key in (b"mem.fail_request", b"mem.fail_malloc", b"mem.fail_scan"):
            assert c.L.hagrid_set_option(c.ctx, key, 1) == EINVAL and "unknown key" in c.error()
            assert c.mem._K.hagrid_kat_set_option(c.ctx, key, -1) == EINVAL
        assert c.mem.mem_pending() == (0, 0, 0)
        assert c.mem._K.hagrid_kat_mem_retry(c.ctx, None) == EINVAL and c.mem.mem_retry()["retries"] == 0
        assert c.mem._K.hagrid_kat_mem_state(c.ctx, None) == EINVAL and c.mem._K.hagrid_kat_mem_state(None, (C.c_int64 * 6)()) == EINVAL
    finally:
        c.close()
