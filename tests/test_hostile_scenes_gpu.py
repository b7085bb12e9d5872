"""The device on the hostile-scene catalogues (tests/_hostile_scenes.py; DESIGN.md section 2, "Admissible scenes").  Flat scenes: the grid arrays after every
construction pass are the CPU oracle's bit for bit, and every query family answers on the device-built grid as the oracle's walk or the family's host
program does.  Scenes with non-finite triangles, boxes that overflow, reference totals beyond 32 bits and depths beyond 23 levels: the documented answer,
the pool as it was, and an ordinary construction right after that equals the oracle's."""
import ctypes as C
import functools

import numpy as np
import pytest

from hagrid_amd import scene

import _closest as K
import _crossings as X
import _hostile_rays as H
import _hostile_scenes as S
import _multi_hit as M
import _overlap as V
from _poison import alloc_out, fetch
from _traverse_formats import IMAGE_FORMATS
from test_build_gpu import assert_same_grid, run_stages
from test_hostile_rays_gpu import World, words

pytestmark = pytest.mark.gpu

FLAT = S.flat_scenes()
NUM_QUERIES = 1024
HAGRID_EINVAL, HAGRID_ERANGE = -1, -4


@pytest.fixture(scope="module")
def mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    """the host programs of the four query families, built once, and the directory they exchange files in"""
    d = tmp_path_factory.mktemp("hostile_scenes_hosts")
    return {"dir": d, "multi": M.build_host(d), "closest": K.build_host(d), "overlap": V.build_host(d), "crossings": X.build_host(d)}


@functools.lru_cache(maxsize=None)
def _world(name, compress):
    from oracle import oracle as O
    tris = FLAT[name]
    return World(tris, O.Grid.full(tris, compress=compress), mesh=False)


class Dev:
    """a flat scene on the device: its triangles, the grid the device built for it (asserted to be the oracle's), the world's batch in a ray buffer"""

    def __init__(self, mem, w, compress):
        from hagrid_amd import api
        self.api, self.mem, self.w = api, mem, w
        self.d_tris = mem.upload(w.tris)
        self.grid = api.build_all(mem, self.d_tris, w.tris.shape[0], compress=compress)
        assert_same_grid(self.grid.download(mem), w.G, "build_all")
        self.d_rays = mem.upload(w.rays)

    def run(self, flags=0, k=0):
        mem, n = self.mem, self.w.n
        count = n * max(k, 1)
        d_hits = alloc_out(mem, 16 * count)
        if k:
            self.api.traverse_grid_multi(self.grid, self.d_tris, self.d_rays, d_hits, n, k, flags)
        else:
            self.api.traverse_grid(self.grid, self.d_tris, self.d_rays, d_hits, n, flags)
        mem.synchronize()
        got = fetch(mem, d_hits, self.api.HIT_DTYPE, count)
        mem.free(d_hits)
        return got

    def close(self):
        self.mem.free(self.d_rays); self.grid.free(); self.mem.free(self.d_tris)


def test_error_codes_are_the_headers():
    from hagrid_amd import lib
    import re, os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hagrid_amd.h")).read()
    codes = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"(HAGRID_E[A-Z]+)\s*=\s*(-\d+)", text))
    assert codes["HAGRID_EINVAL"] == HAGRID_EINVAL and codes["HAGRID_ERANGE"] == HAGRID_ERANGE, codes
    assert lib is not None


@pytest.mark.parametrize("name", list(FLAT))
def test_flat_scene_every_stage_equals_the_oracle(mem, name):
    """build, merge, flatten, expand and compress: the arrays after each pass, bit for bit"""
    grid, G, d_tris = run_stages(mem, FLAT[name])
    assert grid.summary() == G.summary()
    grid.free(); mem.free(d_tris)


@pytest.mark.parametrize("fmt_name", list(IMAGE_FORMATS))
@pytest.mark.parametrize("compress", [False, True], ids=["cell", "small"])
@pytest.mark.parametrize("name", list(FLAT))
def test_flat_scene_nearest_hit_on_every_format_and_variant(mem, name, compress, fmt_name):
    """the oracle's records bit for bit from variants 1, 2, 4 and the default dispatch, with and without ray binning, on every traversal-image format"""
    from hagrid_amd import api
    fmt, slim, general = IMAGE_FORMATS[fmt_name]
    w = _world(name, compress)
    dev = Dev(mem, w, compress)
    try:
        mem.set_option("traverse.image", fmt); mem.set_option("traverse.image_slim", slim); mem.set_option("traverse.image_general", general)
        for variant in (1, 2, 4, 0):
            mem.set_option("traverse.variant", variant)
            api.setup_traversal(dev.grid)
            for binning in (0, 1):
                mem.set_ray_binning(binning)
                w.check(dev.run(), f"{name} {fmt_name} variant={variant} binning={binning}")
    finally:
        mem.set_ray_binning(0); mem.set_option("traverse.variant", 0); mem.set_option("traverse.image", 2)
        mem.set_option("traverse.image_slim", 1); mem.set_option("traverse.image_general", 1)
        dev.close()


@pytest.mark.parametrize("compress", [False, True], ids=["cell", "small"])
@pytest.mark.parametrize("name", list(FLAT))
def test_flat_scene_any_hit_barycentrics_and_multi_hit(mem, name, compress, hosts):
    """any-hit and barycentric records against traverse_ex of the oracle; the k nearest hits, k = 1 and 8, against tests/cpp/multi_hit_host.cpp over the
    same grid arrays"""
    from hagrid_amd import api
    from oracle import oracle as O
    w = _world(name, compress)
    dev = Dev(mem, w, compress)
    try:
        api.setup_traversal(dev.grid)
        for flags, oflags in ((api.UVS, O.UVS), (api.ANY_HIT, O.ANY_HIT), (api.ANY_HIT | api.UVS, O.ANY_HIT | O.UVS)):
            want = w.G.traverse_ex(w.tris, w.rays, oflags, nthreads=8)
            got = dev.run(flags)
            assert (words(got) == words(want)).all(), (name, flags)
            assert (words(got[w.inadmissible]) == H.contract_records(w.rays[w.inadmissible])).all(), (name, flags)
        exe, tmp_path = hosts["multi"], hosts["dir"]
        arrays = dev.grid.download(mem)
        for k in (1, 8):
            want = M.host_walk(exe, tmp_path, arrays, w.tris, w.rays, k)
            got = dev.run(k=k).reshape(w.n, k)
            bad = (got["id"] != want["id"]).any(axis=1) | (M.bits(got["t"]) != M.bits(want["t"])).any(axis=1)
            assert not bad.any(), f"{name} k={k}: {bad.sum()} of {bad.size} rays differ, first at {np.flatnonzero(bad)[:5]}"
            assert (got["u"] == 0).all() and (got["v"] == 0).all()
    finally:
        dev.close()


def _queries(w):
    """1024 points, boxes and rays around a flat scene: the grid's box enlarged by a tenth of its largest extent"""
    lo, hi = np.asarray(w.G.bbox_min, np.float32), np.asarray(w.G.bbox_max, np.float32)
    e = np.float32(0.1) * (hi - lo).max()
    pts = lo - e + scene._uniform_rows(S.SEED + 60, NUM_QUERIES, 3) * (hi - lo + np.float32(2) * e)
    q = np.empty((NUM_QUERIES, 4), np.float32); q[:, 0:3] = pts; q[:, 3] = np.inf
    q[::4, 3] = np.float32(0.05) * (hi - lo).max()
    edge = (np.float32(0.02) + np.float32(0.2) * scene._uniform_rows(S.SEED + 61, NUM_QUERIES, 1)[:, 0]) * (hi - lo).max()
    boxes = V.boxes_around(pts, edge.astype(np.float32))
    rays = scene.make_rays_incoherent(lo - e, hi + e, NUM_QUERIES, S.SEED + 62)
    return np.ascontiguousarray(q), np.ascontiguousarray(boxes), np.ascontiguousarray(rays)


@pytest.mark.parametrize("compress", [False, True], ids=["cell", "small"])
@pytest.mark.parametrize("name", list(FLAT))
def test_flat_scene_closest_overlap_and_crossing_queries(mem, name, compress, hosts):
    """closest-point, box-overlap and crossing queries, 1024 each, against the host programs of the three families over the same grid arrays"""
    from hagrid_amd import api
    w = _world(name, compress)
    dev = Dev(mem, w, compress)
    q, boxes, rays = _queries(w)
    n = NUM_QUERIES
    tmp_path = hosts["dir"]
    surfaces = name not in ("point", "line")              # (zero-area triangles have no surface: no nearest point, no crossing)
    try:
        arrays = dev.grid.download(mem)
        # closest points
        d_q = mem.upload(q); d_res = alloc_out(mem, 32 * n)
        api.closest_points(dev.grid, dev.d_tris, d_q, d_res, n)
        mem.synchronize()
        got = fetch(mem, d_res, api.CLOSEST_DTYPE, n)
        want, _ = K.host_walk(hosts["closest"], tmp_path, arrays, w.tris, q)
        K.assert_results_equal(got, want, f"{name}: closest points against the host walk")
        assert (want["id"] >= 0).sum() > n // 2 or not surfaces
        mem.free(d_q); mem.free(d_res)
        # box overlap, k = 8
        d_b = mem.upload(boxes); d_ids = alloc_out(mem, 4 * 8 * n); d_cnt = alloc_out(mem, 4 * n)
        api.overlap_boxes(dev.grid, dev.d_tris, d_b, n, 8, d_ids, d_cnt)
        mem.synchronize()
        ids = fetch(mem, d_ids, np.int32, 8 * n).reshape(n, 8); cnt = fetch(mem, d_cnt, np.int32, n)
        w_ids, w_cnt, _ = V.host_walk(hosts["overlap"], tmp_path, arrays, w.tris, boxes, 8)
        V.assert_answers_equal(ids, cnt, w_ids, w_cnt, f"{name}: box overlap against the host walk")
        assert (w_cnt > 0).any()
        mem.free(d_b); mem.free(d_ids); mem.free(d_cnt)
        # crossings of rays, inside votes of points
        exe = hosts["crossings"]
        d_r = mem.upload(rays); d_rec = alloc_out(mem, 16 * n)
        api.count_crossings(dev.grid, dev.d_tris, d_r, d_rec, n)
        mem.synchronize()
        rec = fetch(mem, d_rec, np.uint32, 4 * n).reshape(n, 4)
        X.assert_records_equal(rec, X.host_query(exe, tmp_path, w.tris, grid=arrays, page=8, rays=rays)["records"], f"{name}: crossings against the host walk")
        mem.free(d_r); mem.free(d_rec)
        d_p = mem.upload(q); d_in = alloc_out(mem, 4 * n); d_rec = alloc_out(mem, 16 * n * 3)
        api.points_inside(dev.grid, dev.d_tris, d_p, n, d_in, None, d_rec)
        mem.synchronize()
        inside = fetch(mem, d_in, np.int32, n); rec = fetch(mem, d_rec, np.uint32, 4 * n * 3).reshape(n * 3, 4)
        hw = X.host_query(exe, tmp_path, w.tris, grid=arrays, page=8, points=q)
        X.assert_records_equal(rec, hw["records"], f"{name}: point records against the host walk")
        assert (inside == hw["inside"]).all()
        mem.free(d_p); mem.free(d_in); mem.free(d_rec)
    finally:
        dev.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------

def _refused(mem, tris, code, top=S.TOP_DENSITY, snd=S.SND_DENSITY):
    """hagrid_build_grid answers `code`, leaves the grid empty and the pool as it was; returns the message"""
    from hagrid_amd import api, lib
    d_tris = mem.upload(np.ascontiguousarray(tris, np.float32))
    before = mem.usage()
    grid = api.Grid()
    L = lib.load()
    rc = L.hagrid_build_grid(mem._ctx, C.c_void_p(d_tris), tris.shape[0], C.byref(grid.pod), top, snd)
    msg = L.hagrid_last_error(mem._ctx).decode()
    assert rc == code, (rc, msg)
    assert not grid.entries and not grid.cells and not grid.ref_ids
    assert mem.usage() == before, "a refusal changed the pool's usage"
    mem.free(d_tris)
    return msg


def _clean_build_equals_the_oracle(mem):
    from hagrid_amd import api
    from oracle import oracle as O
    tris = S.clean_soup()
    d_tris = mem.upload(tris)
    grid = api.Grid()
    api.build_grid(mem, d_tris, tris.shape[0], grid, S.TOP_DENSITY, S.SND_DENSITY)
    assert_same_grid(grid.download(mem), O.Grid.build(tris), "the clean soup after a refusal")
    grid.free(); mem.free(d_tris)


NONFINITE = S.nonfinite_scenes()


@pytest.mark.parametrize("case", NONFINITE, ids=[c[0] for c in NONFINITE])
def test_nonfinite_scenes_are_refused(mem, case):
    """EINVAL, naming the offending triangle, for an inadmissible triangle wherever it stands; ERANGE for finite triangles whose extent overflows"""
    name, tris, answer, row = case
    msg = _refused(mem, tris, HAGRID_EINVAL if answer == S.EINVAL else HAGRID_ERANGE)
    if row is not None:
        assert f"triangle {row} " in msg, msg
    elif answer == S.EINVAL:
        assert "triangle 0 " in msg, msg
    _clean_build_equals_the_oracle(mem)


def test_nan_vertex_through_scene_assemble(mem):
    """a NaN vertex that reaches the triangles through hagrid_scene_assemble: the construction refuses the assembled buffer, and accepts it once the vertex is finite"""
    from hagrid_amd import api
    verts, faces = scene.make_stadium_mesh(0.05)
    verts = np.ascontiguousarray(verts, np.float32).copy(); faces = np.ascontiguousarray(faces, np.int32)
    bad = verts.copy(); bad[int(faces[11, 1]), 2] = np.nan
    from hagrid_amd import lib
    nt = faces.shape[0]
    d_faces = mem.upload(faces)
    for v, code in ((bad, HAGRID_EINVAL), (verts, 0)):
        d_verts = mem.upload(v)
        ms = api.MeshScene(mem, [(d_verts, v.shape[0], d_faces, nt)])
        assert ms.num_tris == nt
        d_tris = mem.alloc(48 * nt)
        ms.assemble(0, d_tris)
        mem.synchronize()
        before = mem.usage()
        grid = api.Grid()
        rc = lib.load().hagrid_build_grid(mem._ctx, C.c_void_p(d_tris), nt, C.byref(grid.pod), S.TOP_DENSITY, S.SND_DENSITY)
        msg = lib.load().hagrid_last_error(mem._ctx).decode()
        assert rc == code, (rc, msg)
        if rc == 0:
            grid.mem = mem; grid.free()
        else:
            got = mem.download(d_tris, np.float32, 12 * nt).reshape(nt, 12)
            first_bad = int(np.flatnonzero(~np.isfinite(got).all(axis=1))[0])
            assert f"triangle {first_bad} " in msg, (msg, first_bad)
        assert mem.usage() == before
        ms.close(); mem.free(d_tris); mem.free(d_verts)
    mem.free(d_faces)


@pytest.mark.parametrize("band,tris", S.size_scenes(), ids=[b for b, _ in S.size_scenes()])
def test_reference_totals_beyond_the_limit_are_refused(band, tris):
    """thin slabs whose true top-level total lies in (2^30, 2^31), in (2^31, 2^32), and beyond 2^32 with low 32 bits that a 32-bit sum would accept:
    ERANGE before anything is sized by the total -- the pool's peak stays below what pair_rank alone would take at the wrapped total"""
    from hagrid_amd import api
    total = S.top_reference_total(tris)
    assert S.BANDS[band](total)
    m = api.MemManager(keep=False)
    try:
        msg = _refused(m, tris, HAGRID_ERANGE)
        assert "top-level references" in msg, msg
        wrapped = total % 2 ** 32
        print("band", band, "total", total, "wrapped", wrapped, "pool peak", m.max_usage())
        assert m.max_usage() < 4 * min(wrapped, 2 ** 30)
        _clean_build_equals_the_oracle(m)
    finally:
        m.close()


@pytest.mark.parametrize("snd", [1e22, 1e30])
def test_a_second_level_of_24_levels_is_refused(mem, snd):
    msg = _refused(mem, S.clean_soup(), HAGRID_ERANGE, snd=snd)
    assert "too many levels" in msg, msg
    _clean_build_equals_the_oracle(mem)
