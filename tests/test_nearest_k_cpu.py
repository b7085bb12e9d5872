"""Neighbour queries (hagrid_nearest_tris), the part that needs no GPU: the numpy statement hagrid_amd/scene.py nearest_tris, the header's brute force with
the k-list (tests/cpp/nearest_k_host.cpp) and the fixture tests/golden/nearest_k.npz against each other, bit for bit; the host walk -- the walk the gfx950
kernel runs -- over grids of the CPU oracle against the fixture for several k; k = 1 against the fixture of the nearest-surface query; paging to the end,
page boundaries inside ties, cursor edge cases; labels on a mesh's own vertices; the deep grids of _deep_grids at every stage, once more under
sanitizers; the kernels' resources and the kernel budget; the entry point in header, library and bindings."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _closest as K
import _deep_grids as D
import _host
import _nearest_k as NK
from hagrid_amd import scene

ROOT = K.ROOT
INC = K.INC


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return np.load(NK.FIXTURE)


@pytest.fixture(scope="module")
def closest_fixture():
    return np.load(K.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("nearest_k_host")
    return NK.build_host(d), d


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name in K.SCENES:
        tris = K.make_tris(name)
        out[name] = (tris, K.fixture_queries(tris))
    return out


_GRIDS = {}


def grid_arrays(scenes, name, compress, subset_only):
    key = (name, compress, subset_only)
    if key not in _GRIDS:
        _GRIDS[key] = K.oracle_grid_arrays(K.oracle_grid(scenes[name][0], compress, subset_only))
    return _GRIDS[key]


@pytest.mark.parametrize("name", K.SCENES)
def test_statement_host_brute_force_and_fixture_agree(fixture, scenes, host, name):
    """nearest_k_host brute == scene.nearest_tris == the fixture, entries and records, all 4096 queries at k = 8; the stored pages likewise"""
    exe, d = host
    tris, q = scenes[name]
    assert int(fixture[name + "_query_sum"]) == int(K.bits(q).astype(np.uint64).sum()), "the fixture's queries are the generators' queries"
    want, want_pages = NK.fixture_lists(fixture, name)
    e, r = scene.nearest_tris(tris, q, NK.KMAX)
    be, br = NK.host_brute(exe, d, tris, q, NK.KMAX)
    NK.assert_lists_equal(e, want, f"{name}: scene.nearest_tris against the fixture")
    NK.assert_lists_equal(be, want, f"{name}: brute force of closest.h against the fixture")
    NK.assert_lists_equal(br, r, f"{name}: records of the brute force against the statement")
    qs = q[NK.STORED]
    got = NK.first_pages(lambda cursors: NK.host_brute(exe, d, tris, qs, NK.PAGE_K, cursors=cursors)[0], qs.shape[0])
    NK.assert_lists_equal(got.reshape(-1, NK.PAGE_K), want_pages.reshape(-1, NK.PAGE_K), f"{name}: pages of the brute force against the fixture")
    assert os.path.getsize(NK.FIXTURE) < 400000


def test_fixture_semantics(fixture, scenes):
    for name in K.SCENES:
        tris, q = scenes[name]
        e, _ = NK.fixture_lists(fixture, name)
        used = e["id"] >= 0
        r2 = q[:, 3] * q[:, 3]
        assert (used[:, :-1] >= used[:, 1:]).all(), "used slots come first"
        d_ok = (e["d2"][:, :-1] < e["d2"][:, 1:]) | ((e["d2"][:, :-1] == e["d2"][:, 1:]) & (e["id"][:, :-1] < e["id"][:, 1:]))
        assert (d_ok | ~used[:, 1:]).all(), "sorted by (d2, id), no triangle twice"
        assert (e["d2"][used] <= np.broadcast_to(r2[:, None], e.shape)[used]).all()
        inactive = q[:, 3] < 0
        assert inactive.sum() == 8 and (e["id"][inactive] == -1).all() and (e["d2"][inactive] == -1).all()
        nan = np.isnan(q[:, 0:3]).any(axis=1)
        assert nan.sum() == 8 and (e["id"][nan] == -1).all()
        rest = ~used & ~inactive[:, None]
        assert (K.bits(e["d2"])[rest] == np.broadcast_to(K.bits(r2)[:, None], e.shape)[rest]).all(), "an unused slot holds r2"
        assert 0 < used[K.RADIUS, 0].sum() < 512 and not used[K.RADIUS].all(axis=1).all()


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", K.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, scenes, host, scene_name, compress, subset_only):
    """entries bit-equal for all 4096 queries and k in {1, 2, 3, 5, 8} over Cell and SmallCell grids of the CPU oracle, both expansion modes: the list for k
    is the first k slots of the list for 8; the records are the statement's"""
    exe, d = host
    tris, q = scenes[scene_name]
    arrays = grid_arrays(scenes, scene_name, compress, subset_only)
    want, _ = NK.fixture_lists(fixture, scene_name)
    for k in (1, 2, 3, 5, 8):
        e, r, counts = NK.host_walk(exe, d, arrays, tris, q, k)
        NK.assert_lists_equal(e, want[:, :k], f"{scene_name} compress={compress} subset_only={subset_only} k={k}")
        assert (r["id"] == e["id"]).all() and (K.bits(r["d2"]) == K.bits(e["d2"])).all()
        assert ((e["id"][:, k - 1] >= 0) == (counts[:, 3] != 0)).all()
        trivial = (q[:, 3] < 0) | np.isnan(q[:, 0:3]).any(axis=1)
        assert (counts[trivial] == 0).all() and (counts[~trivial, 0] >= 1).all()
    if not compress and subset_only:
        NK.assert_lists_equal(r[:256], scene.nearest_tris(tris, q[:256], 8)[1], f"{scene_name}: records of the walk against the statement")
        print(scene_name, "triangles tested per query at k = 8:", counts[:, 1].mean())


@pytest.mark.parametrize("scene_name", K.SCENES)
def test_k1_is_the_nearest_surface_query(closest_fixture, fixture, scenes, host, scene_name):
    """k = 1, no cursor, no labels: entries are (d2, id) of tests/golden/closest.npz and records its whole 32 bytes, no query excepted"""
    exe, d = host
    tris, q = scenes[scene_name]
    want = K.fixture_results(closest_fixture, scene_name)
    for compress in (False, True):
        e, r, _ = NK.host_walk(exe, d, grid_arrays(scenes, scene_name, compress, True), tris, q, 1)
        K.assert_results_equal(r[:, 0], want, f"{scene_name} compress={compress}: records at k = 1")
        assert (e["id"][:, 0] == want["id"]).all() and (K.bits(e["d2"][:, 0]) == K.bits(want["d2"])).all()
    pick = np.concatenate([np.arange(s.start, s.stop)[:48] for s in (K.NEAR, K.UNIFORM, K.RADIUS, K.SURFACE, K.VERTEX)] + [np.arange(K.SPECIAL.start, K.SPECIAL.stop)])
    K.assert_results_equal(scene.nearest_tris(tris, q[pick], 1)[1][:, 0], want[pick], f"{scene_name}: the statement at k = 1 (a slice of every section)")


# the queries that must page, counted with the numpy statement: (two or more pages, four or more)
MUST_PAGE = {"soup": (300, 30), "mesh": (50, 30)}


@pytest.mark.parametrize("scene_name", K.SCENES)
def test_paging_to_the_end(fixture, scenes, host, scene_name):
    """k = 3, RADIUS and SPECIAL[32:48], every query paged to its end over a SmallCell grid: the concatenation is scene.tris_within; the first three pages
    are the fixture's"""
    exe, d = host
    tris, q = scenes[scene_name]
    arrays = grid_arrays(scenes, scene_name, True, True)
    qs = q[NK.PAGED]
    lists, pages = NK.page_through(lambda which, cursors: NK.host_walk(exe, d, arrays, tris, qs[which], NK.PAGE_K, cursors=cursors)[0], qs.shape[0], NK.PAGE_K)
    csr = scene.tris_within(tris, qs)
    NK.assert_pages_equal_csr(lists, csr, scene_name)
    sizes = np.diff(csr["offsets"])
    print(scene_name, "queries with >= 3 candidates:", int((sizes >= 3).sum()), ">= 9:", int((sizes >= 9).sum()), "longest:", int(sizes.max()))
    assert (pages == sizes // NK.PAGE_K + 1).all()
    two, four = MUST_PAGE[scene_name]
    assert (pages >= 2).sum() >= two and (pages >= 4).sum() >= four, "the lists must page"
    _, want_pages = NK.fixture_lists(fixture, scene_name)
    qf = q[NK.STORED]
    got = NK.first_pages(lambda cursors: NK.host_walk(exe, d, arrays, tris, qf, NK.PAGE_K, cursors=cursors)[0], qf.shape[0])
    NK.assert_lists_equal(got.reshape(-1, NK.PAGE_K), want_pages.reshape(-1, NK.PAGE_K), f"{scene_name}: pages of the walk against the fixture")


def test_cursor_inside_a_tie(fixture, scenes, host):
    """the mesh: the 192 VERTEX queries and SPECIAL[32:40] (vertices with r = 0, 4 to 6 candidates, all at d2 = 0) have several triangles at the same d2; at
    k = 3 the page boundary falls inside the tie: the three pages hold every id once, ascending inside the tie -- the first nine of the statement's list"""
    exe, d = host
    tris, q = scenes["mesh"]
    arrays = grid_arrays(scenes, "mesh", False, True)
    pick = np.concatenate([np.arange(K.VERTEX.start, K.VERTEX.stop), np.arange(K.SPECIAL.start + 32, K.SPECIAL.start + 40)])
    qs = q[pick]
    pages = NK.first_pages(lambda cursors: NK.host_walk(exe, d, arrays, tris, qs, NK.PAGE_K, cursors=cursors)[0], qs.shape[0])
    want, _ = scene.nearest_tris(tris, qs, NK.PAGE_K * NK.PAGES)
    got = np.concatenate(list(pages), axis=1)                # (n, 9): page after page
    vertex = np.arange(192)
    NK.assert_lists_equal(got[vertex], want[vertex], "VERTEX: three pages against the first nine of the statement")
    inside = 0
    for i in range(qs.shape[0]):
        l = got[i][got[i]["id"] >= 0]
        if i >= 192:                                         # r = 0: the list ends on the second page; the third repeats it (the cursor was kept)
            l = l[:(want["id"][i] >= 0).sum()]
            assert 4 <= l.size <= 6 and (l["d2"] == 0).all() and (l == want[i][:l.size]).all()
        assert np.unique(l["id"]).size == l.size, "every id once"
        tie = l["d2"][1:] == l["d2"][:-1]
        assert (np.diff(l["id"])[tie] > 0).all(), "ascending inside a tie"
        inside += bool(l.size > NK.PAGE_K and l["d2"][NK.PAGE_K - 1] == l["d2"][NK.PAGE_K])
    assert inside >= 8, "at least 8 queries page inside a tie"
    print("queries whose first page boundary falls inside a tie:", inside)


def test_cursor_edge_cases(fixture, scenes, host):
    """a cursor of d2 = -1 excludes nothing (whatever its id), a cursor with a NaN d2 excludes everything"""
    exe, d = host
    tris, q = scenes["soup"]
    arrays = grid_arrays(scenes, "soup", True, True)
    qs = q[K.RADIUS]
    want, _ = NK.fixture_lists(fixture, "soup")
    n = qs.shape[0]
    for cid in (-1, 0, 2 ** 31 - 1):
        cur = NK.entries_of(np.full(n, -1.0, np.float32), np.full(n, cid, np.int32))
        NK.assert_lists_equal(NK.host_walk(exe, d, arrays, tris, qs, 8, cursors=cur)[0], want[K.RADIUS], f"cursor (-1, {cid})")
        NK.assert_lists_equal(scene.nearest_tris(tris, qs[:64], 8, cursors=cur[:64])[0], want[K.RADIUS][:64], f"statement, cursor (-1, {cid})")
    cur = NK.entries_of(np.full(n, np.nan, np.float32), np.full(n, -1, np.int32))
    for e in (NK.host_walk(exe, d, arrays, tris, qs, 8, cursors=cur)[0], scene.nearest_tris(tris, qs[:64], 8, cursors=cur[:64])[0], NK.host_brute(exe, d, tris, qs, 8, cursors=cur)[0]):
        assert (e["id"] == -1).all() and (K.bits(e["d2"]) == K.bits(qs[:e.shape[0], 3] * qs[:e.shape[0], 3])[:, None]).all()


def test_labels_on_the_meshs_own_vertices(host):
    """the stadium mesh, its vertices as queries with label = vertex index and the index triples as triangle labels: the walk is the statement, and the
    unlabelled statement over the scene without the vertex's incident triangles; no list holds an incident triangle; without labels the first entries
    ARE the incident triangles at d2 = 0; a label of -1 skips nothing"""
    exe, d = host
    tris, F, q, labels = NK.stadium_labels()
    G = K.oracle_grid(tris, True, True)
    arrays = K.oracle_grid_arrays(G)
    k = 8
    e, r, _ = NK.host_walk(exe, d, arrays, tris, q, k, query_labels=labels, tri_labels=F)
    se, sr = scene.nearest_tris(tris, q, k, query_labels=labels, tri_labels=F)
    NK.assert_lists_equal(e, se, "labelled walk against the statement")
    NK.assert_lists_equal(r, sr, "labelled walk against the statement: records")
    NK.assert_lists_equal(NK.host_brute(exe, d, tris, q, k, query_labels=labels, tri_labels=F)[0], se, "labelled brute force against the statement")
    incident = (F[e["id"].clip(0)] == labels[:, None, None]).any(axis=2) & (e["id"] >= 0)
    assert not incident.any(), "a list holds a triangle the vertex belongs to"
    assert (e["id"] >= 0).any(axis=1).sum() > q.shape[0] // 2, "most vertices have neighbours they do not belong to"
    # the scene with each vertex's incident triangles removed (their stored normal cleared: no surface, ids unchanged), a slice of the vertices
    for v in range(0, q.shape[0], max(1, q.shape[0] // 96)):
        t2 = tris.copy()
        t2[(F == v).any(axis=1)] = t2[(F == v).any(axis=1)] * np.float32([1, 1, 1, 0] * 3)
        NK.assert_lists_equal(scene.nearest_tris(t2, q[v:v + 1], k)[0], e[v:v + 1], f"vertex {v}: the unlabelled statement without its triangles")
    # without labels, and with labels of -1: the incident triangles come first, at d2 = 0
    plain, _, _ = NK.host_walk(exe, d, arrays, tris, q, k)
    minus, _, _ = NK.host_walk(exe, d, arrays, tris, q, k, query_labels=np.full(q.shape[0], -1, np.int32), tri_labels=F)
    NK.assert_lists_equal(minus, plain, "labels of -1 skip nothing")
    # (a vertex may also touch triangles it does not belong to -- the floor under a pillar -- so the incident ones are among the first entries, not
    # alone there; and d2 is exactly 0 where the vertex is the triangle's stored v0: v1 and v2 are made again as v0 - e1, v0 + e2)
    has_surface = ~((tris[:, 3] == 0) & (tris[:, 7] == 0) & (tris[:, 11] == 0))
    is_v0 = np.zeros(q.shape[0], dtype=bool); is_v0[F[has_surface, 0]] = True
    incident = (F[plain["id"].clip(0)] == labels[:, None, None]).any(axis=2) & (plain["id"] >= 0)
    assert is_v0.sum() > q.shape[0] // 2
    assert (plain["d2"][is_v0, 0] == 0).all() and (incident & (plain["d2"] == 0)).any(axis=1)[is_v0].all(), "without labels a vertex finds its own triangles first"
    assert incident.any(axis=1).sum() >= is_v0.sum() and incident.sum() > 3 * q.shape[0]
    assert (plain["id"] != e["id"]).any()


@pytest.fixture(scope="module")
def deep_hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("nearest_k_deep")
    return {"plain": NK.build_host(d), "san": NK.build_host(d, sanitize=True), "dir": d}


@pytest.mark.parametrize("name", D.WALKED)
def test_deep_grids_at_every_stage(deep_hosts, name):
    """every scene and stage of _deep_grids.CATALOGUE: the host walk at k = 8 against the host brute force, bit for bit; once more with the stand-alone
    sanitizer build of the host program"""
    d = deep_hosts["dir"]
    tris = D.make_tris(name)
    pts = D.points(tris)
    want_e, want_r = NK.host_brute(deep_hosts["plain"], d, tris, pts, 8)
    assert ((want_e["id"] >= 0).sum(axis=1) >= 2).sum() > D.NUM_POINTS // 4 and (want_e["id"][:, -1] < 0).any()
    st = D.OracleStages(name, tris)
    for stage in D.stages_of(name):
        out = D.stage_grid(st, stage)
        G = out[0] if stage == "compress" else out
        arrays = _host.oracle_grid_arrays(G)
        for which in ("plain", "san"):
            e, r, _ = NK.host_walk(deep_hosts[which], d, arrays, tris, pts, 8)
            NK.assert_lists_equal(e, want_e, f"{name} after {stage} ({which})")
            NK.assert_lists_equal(r, want_r, f"{name} after {stage} ({which}): records")


def test_kernel_resources_and_budget(fixture):
    """tools/kernel_resources.py closest: no scratch and no spill for both kernels, 94 VGPRs for closest_points_kernel (the template costs the existing
    query nothing); tools/count_kernels.py: at most 120 kernels"""
    rows = _host.kernel_rows("closest")
    assert set(rows) == {"closest_points_kernel", "nearest_tris_kernel"}, rows
    for name, (vgpr, spill, scratch, occ) in rows.items():
        assert spill == 0 and scratch == 0, (name, rows[name])
    assert rows["closest_points_kernel"][0] == 94 and rows["closest_points_kernel"][3] == 5
    assert rows["nearest_tris_kernel"][0] <= 128 and rows["nearest_tris_kernel"][3] >= 4
    c = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "count_kernels.py")], capture_output=True, text=True, cwd=ROOT)
    m = re.search(r"(\d+) kernels", c.stdout)
    assert m and int(m.group(1)) <= 120, c.stdout[-300:] + c.stderr[-300:]


def test_records_and_entry_point(fixture):
    """the ctypes mirror: record sizes, the symbol declared in the header, exported by the library and bound"""
    from hagrid_amd import api, lib
    assert scene.NEAREST_ENTRY_DTYPE.itemsize == 8 and [scene.NEAREST_ENTRY_DTYPE.fields[k][1] for k in ("d2", "id")] == [0, 4]
    assert api.NEAREST_ENTRY_DTYPE is scene.NEAREST_ENTRY_DTYPE and api.MAX_NEAREST == 8
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "hagrid_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+hagrid_nearest_tris\s*\(", code) and re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", code)
    assert re.search(r"#define\s+HAGRID_MAX_NEAREST\s+8\b", code)
    L = lib.load()
    assert "hagrid_nearest_tris" in lib.SIGNATURES and hasattr(L, "hagrid_nearest_tris") and len(lib.SIGNATURES["hagrid_nearest_tris"][1]) == 13
    for name in ("nearest_tris", "tris_within", "MAX_NEAREST"):
        assert hasattr(api, name) and name in api.__all__
    prog = '#include "hagrid_amd.h"\nint main(void) { return sizeof(&hagrid_nearest_tris) ? 0 : 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-fsyntax-only", "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
