"""Contact queries (hagrid_overlap_tris), the part that needs no GPU.  The yardstick is exact arithmetic (tests/_overlap_tris.py exact_meet, stored by
tests/golden/make_golden_overlap_tris.py in tests/golden/overlap_tris.npz): tri_meets of include/hagrid/tri_tri.h (compiled for the host) and
scene.tri_tri_pairs on lattice pairs, where float32 is exact; the full pair decision on pairs of neighbouring triangles of two scenes, where it may err by
rounding in one direction only; the host walk tests/cpp/overlap_tris_host.cpp -- the walk the gfx950 kernel runs -- over grids of the CPU oracle against the
host brute force, the numpy statement and the fixture, for k = 1, 2, 3, 4, 5, 8, both cell formats and both expansion modes; a lattice scene against the
exact test alone; ANY; paging; labels; the host program under the sanitizers; the entry point in header, library and bindings."""
import os
import re
import subprocess

import numpy as np
import pytest

import _host
import _overlap_tris as W
from hagrid_amd import scene

ROOT = W.ROOT


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return np.load(W.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_tris_host")
    return W.build_host(d), d


@pytest.fixture(scope="module")
def scenes(fixture):
    """name -> (tris, queries, first, query_labels, tri_labels)"""
    out = {}
    for name in W.SCENES:
        tris = W.make_tris(name)
        out[name] = (tris, *W.scene_queries(fixture, name, tris), W.scene_labels(name, tris.shape[0]))
    return out


@pytest.fixture(scope="module")
def lattice(fixture):
    tris, queries, _, _ = W.lattice_scene()
    assert W.array_sum(tris) + W.array_sum(queries) == int(fixture["lattice_scene_sum"])
    return tris, queries


def members(tris, queries, ids, first=None, query_labels=None, tri_labels=None):
    """is ids[i] (>= 0) a member of S_i, by the numpy statement of every condition?"""
    glo, ghi = scene.grid_box(tris)
    boxes = scene.clip_boxes(scene.query_boxes(queries, glo, ghi), glo, ghi)
    ok = scene.overlap_pairs(tris[ids], boxes) & scene.tri_tri_pairs(queries, tris[ids]) & scene.tris_have_surface(tris[ids])
    if first is not None:
        ok &= ids >= first
    if query_labels is not None:
        ok &= ~scene.labels_shared(query_labels, tri_labels[ids])
    return ok


def test_lattice_pairs_equal_the_exact_test(fixture, host):
    """(a): tri_meets through the host program and scene.tri_tri_pairs equal the exact truth on all 16 384 lattice pairs -- a quarter coplanar, where a
    predicate without the six in-plane axes calls every pair a contact"""
    exe, d = host
    a, b, _ = W.lattice_pairs()
    assert a.shape[0] == W.NUM_LATTICE_PAIRS and W.array_sum(a) + W.array_sum(b) == int(fixture["lattice_pair_sum"])
    assert np.abs(scene.tri_vertices(a)).max() <= 16 and np.abs(scene.tri_vertices(b)).max() <= 16
    truth = np.unpackbits(fixture["lattice_truth"])[:W.NUM_LATTICE_PAIRS].astype(bool)
    got = scene.tri_tri_pairs(a, b)
    assert (got == truth).all(), f"scene.tri_tri_pairs: {(got != truth).sum()} of {truth.size} pairs differ from the exact test, first at {np.flatnonzero(got != truth)[:5]}"
    got = W.host_pairs(exe, d, a, b)
    assert (got == truth).all(), f"tri_meets: {(got != truth).sum()} of {truth.size} pairs differ from the exact test, first at {np.flatnonzero(got != truth)[:5]}"
    q = W.NUM_LATTICE_PAIRS // 4
    assert 200 < truth[:q].sum() < q - 200 and (~truth[q:q + q // 2]).sum() > 200 and truth[q + q // 2:].sum() > 200, "both answers occur in every class"
    assert (W.host_pairs(exe, d, b, a) == truth).all(), "the pair is symmetric"


def test_scene_pairs_err_by_rounding_in_one_direction(fixture, host):
    """(b): on pairs of triangles whose boxes come within 2 eps of each other the full pair decision (grown-box test AND tri_meets) never says "apart" where
    the exact test says "meet" -- but for the pairs the fixture lists as contacts at rounding distance, at most 0.1 % --, and says "meet" where the exact test
    says "apart" for at most 1 % of a scene's pairs"""
    exe, d = host
    for name in W.SCENES:
        tris = W.make_tris(name)
        pairs = fixture[name + "_pairs"]
        assert pairs.shape == (W.NUM_SCENE_PAIRS, 2) and (pairs[:, 0] != pairs[:, 1]).all()
        truth = np.unpackbits(fixture[name + "_pairs_truth"])[:W.NUM_SCENE_PAIRS].astype(bool)
        listed = fixture[name + "_pairs_rounding"]
        assert listed.size <= W.NUM_SCENE_PAIRS // 1000
        got = W.pair_decision(tris, pairs)
        assert (W.host_pairs(exe, d, tris[pairs[:, 0]], tris[pairs[:, 1]]) == scene.tri_tri_pairs(tris[pairs[:, 0]], tris[pairs[:, 1]])).all(), "header and numpy agree"
        apart = truth & ~got
        apart[listed] = False
        false_meets = int((got & ~truth).sum())
        print(f"{name}: {truth.sum()} of {truth.size} pairs meet exactly; apart where exact says meet: {int((truth & ~got).sum())} ({listed.size} listed); meet where exact says apart: {false_meets}")
        assert not apart.any(), f"{name}: {apart.sum()} pairs that meet exactly are called apart, first at {np.flatnonzero(apart)[:5]}"
        assert false_meets <= W.NUM_SCENE_PAIRS // 100
        assert truth.sum() > 400 and (~truth).sum() > 400


def test_fixture_is_the_statement_and_the_brute_force(fixture, scenes, host):
    """(c): the stored answers are what the header's brute force gives (k = 8 and k = 1, with and without labels) and what scene.overlap_tris gives"""
    exe, d = host
    for name in W.SCENES:
        tris, q, first, qlab, tlab = scenes[name]
        for key, labels in ((name, (None, None)), (name + "_lab", (qlab, tlab))):
            for k in (W.KMAX, 1):
                ids, counts = W.host_brute(exe, d, tris, q, k, first, *labels)
                W.assert_answers_equal(ids, counts, *W.expected(fixture, key, k), f"{key} k={k}: the brute force")
            r = scene.overlap_tris(tris, q, k=W.KMAX, first=first, query_labels=labels[0], tri_labels=labels[1])
            W.assert_answers_equal(r["ids"], r["counts"], *W.expected(fixture, key, W.KMAX), f"{key}: scene.overlap_tris")
            assert (r["sizes"] == fixture[key + "_sizes"]).all()
        ids, counts = W.host_brute(exe, d, tris, q, 3)
        W.assert_answers_equal(ids, counts, *W.expected(fixture, name, 3, first=False), f"{name} without first")


def test_fixture_semantics(fixture, scenes):
    for name in W.SCENES:
        tris, q, first, qlab, tlab = scenes[name]
        for key in (name, name + "_lab"):
            ids, sizes = fixture[key + "_ids"], fixture[key + "_sizes"]
            listed = ids >= 0
            assert (listed.sum(axis=1) == np.minimum(sizes, W.KMAX)).all(), "min(k, m) slots are used"
            assert (listed[:, :-1] >= listed[:, 1:]).all(), "the unused slots are the last ones"
            both = listed[:, :-1] & listed[:, 1:]
            assert (ids[:, 1:][both] > ids[:, :-1][both]).all() and ids.max() < tris.shape[0], "ascending, each id once"
            assert (sizes[W.BEYOND] == 0).all() and (sizes[W.INACTIVE] == 0).all() and (ids[W.INACTIVE] == -1).all()
            assert (sizes[W.HUGE] > W.KMAX + 1).sum() > 64 and (sizes[W.MOVED] > 0).sum() > 100 and (sizes[W.FLAT] > 0).sum() > 100
            for k in W.KS:
                assert (sizes < k).any() and (sizes == k).any() and (sizes == k + 1).any() and (sizes > k + 1).any(), (key, k)
        assert not scene.tris_admissible(q[W.INACTIVE]).all() and (~scene.tris_admissible(q[W.INACTIVE])).sum() == 64
        plain, lab = fixture[name + "_sizes"], fixture[name + "_lab_sizes"]
        assert (plain[W.OWN] >= 1).all(), "without labels a triangle of the scene finds itself"
        assert (lab[W.OWN] < plain[W.OWN]).all() and (lab[W.OWN.stop:] == plain[W.OWN.stop:]).all(), "labels leave out the triangle itself (and its neighbours); queries without labels keep their answers"
        src = fixture[name + "_ids"][W.PAGED_FROM:W.PAGED_FROM + 128]
        assert (first[W.PAGED] == src[:, 2] + 1).all() and (first[W.PAGED] > 0).sum() >= 64 and (first[:W.PAGED.start] == 0).all()
        paged = fixture[name + "_ids"][W.PAGED]
        full = src[:, 2] >= 0
        assert (paged[full, :5] == src[full, 3:]).all(), "the page after the third id starts with the fourth"


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", W.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, scenes, host, scene_name, compress, subset_only):
    """(c): ids and counts of all 4096 queries for k = 1, 2, 3, 4, 5, 8 over Cell and SmallCell grids of the CPU oracle, both expansion modes -- with first
    and labels, with first alone, with neither; the prefix property; ANY; inactive queries take no walk"""
    exe, d = host
    tris, q, first, qlab, tlab = scenes[scene_name]
    G = W.oracle_grid(tris, compress, subset_only)
    assert (G.small_cells is not None) == compress
    arrays = W.oracle_grid_arrays(G)
    what = f"{scene_name} compress={compress} subset_only={subset_only}"
    prev = None
    for k in W.KS:
        ids, counts, totals = W.host_walk(exe, d, arrays, tris, q, k, first, qlab, tlab)
        W.assert_answers_equal(ids, counts, *W.expected(fixture, scene_name + "_lab", k), f"{what} k={k} with labels")
        assert (totals[W.INACTIVE] == 0).all() and (totals[W.BEYOND, 1] == 0).all()
        if prev is not None:
            assert (ids[:, :prev.shape[1]] == prev).all(), "the prefix property"
        prev = ids
    for k in (W.KMAX, 2):
        ids, counts, _ = W.host_walk(exe, d, arrays, tris, q, k, first)
        W.assert_answers_equal(ids, counts, *W.expected(fixture, scene_name, k), f"{what} k={k} with first")
    ids, counts, _ = W.host_walk(exe, d, arrays, tris, q, 4)
    W.assert_answers_equal(ids, counts, *W.expected(fixture, scene_name, 4, first=False), f"{what} k=4 with neither")
    # ANY: some member of S exactly where S is not empty
    for key, labels in ((scene_name, (None, None)), (scene_name + "_lab", (qlab, tlab))):
        ids, counts, totals = W.host_walk(exe, d, arrays, tris, q, 1, first, *labels, any_=True)
        sizes = fixture[key + "_sizes"]
        assert ((ids[:, 0] >= 0) == (sizes > 0)).all() and (counts == (sizes > 0)).all() and (ids[sizes == 0, 0] == -1).all()
        hit = ids[:, 0] >= 0
        lab = (None, None) if labels[0] is None else (qlab[hit], tlab)
        assert members(tris, q[hit], ids[hit, 0], first[hit], *lab).all(), "ANY returns a member of S"


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
def test_lattice_scene_equals_the_exact_test(fixture, lattice, host, compress, subset_only):
    """(d): 4000 lattice triangles, 1024 lattice queries: the host walk, the host brute force and the numpy statement all give what the exact test ALONE gives"""
    exe, d = host
    tris, queries = lattice
    arrays = W.oracle_grid_arrays(W.oracle_grid(tris, compress, subset_only))
    sizes = fixture["lattice_sizes"]
    assert sizes.size == W.LATTICE_QUERIES and (sizes == 0).any() and (sizes > W.KMAX + 1).any()
    for k in W.KS:
        want = W.expected(fixture, "lattice", k)
        ids, counts, _ = W.host_walk(exe, d, arrays, tris, queries, k)
        W.assert_answers_equal(ids, counts, *want, f"lattice scene compress={compress} subset_only={subset_only} k={k}: the walk")
        if not compress and subset_only:
            ids, counts = W.host_brute(exe, d, tris, queries, k)
            W.assert_answers_equal(ids, counts, *want, f"lattice scene k={k}: the brute force")
    ids, counts, _ = W.host_walk(exe, d, arrays, tris, queries, 1, any_=True)
    assert ((ids[:, 0] >= 0) == (sizes > 0)).all() and (counts == (sizes > 0)).all()
    if compress and not subset_only:
        r = scene.overlap_tris(tris, queries, k=W.KMAX)
        W.assert_answers_equal(r["ids"], r["counts"], *W.expected(fixture, "lattice", W.KMAX), "lattice scene: scene.overlap_tris")
        assert (r["sizes"] == sizes).all()


def test_paging_reproduces_the_whole_list(scenes, host):
    """k = 3 and first = last id + 1, again and again, gives the whole brute-force list of 192 queries of the mesh, in order"""
    exe, d = host
    tris, q, _, _, _ = scenes["mesh"]
    pick = np.concatenate([np.arange(W.OWN.start, W.OWN.start + 96), np.arange(W.FLAT.start, W.FLAT.start + 96)])
    qq = q[pick]
    n = qq.shape[0]
    arrays = W.oracle_grid_arrays(W.oracle_grid(tris, True, False))
    whole = scene.overlap_tris(tris, qq, k=256)
    assert whole["sizes"].max() <= 256 and whole["sizes"].max() > 20
    pages = [[] for _ in range(n)]
    live = np.arange(n)
    first = np.zeros(n, dtype=np.int32)
    for _ in range(100):
        ids, counts, _ = W.host_walk(exe, d, arrays, tris, qq[live], 3, first[live])
        for row, i in enumerate(live):
            pages[i] += [int(v) for v in ids[row] if v >= 0]
        more = counts == 4
        assert (counts[~more] == (ids[~more] >= 0).sum(axis=1)).all()
        first[live[more]] = ids[more, 2] + 1
        live = live[more]
        if live.size == 0:
            break
    assert live.size == 0
    for i in range(n):
        assert pages[i] == [int(v) for v in whole["ids"][i, :whole["sizes"][i]]], f"query {pick[i]}"


def test_labels(host):
    """A closed solid against itself: with its faces as labels nothing is left (a triangle touches its neighbours only); without labels every triangle
    reports itself and every neighbour that shares a vertex; first[i] = i + 1 gives every pair exactly once -- compared with the numpy pair matrix"""
    exe, d = host
    verts, faces, solids = scene.make_stadium_mesh(0.05, solids_only=True)
    for solid in (solids[0], solids[4], solids[-1]):               # a torus, a sphere, a lamp
        f0, nf = solid["faces"]
        labels = np.ascontiguousarray(faces[f0:f0 + nf], np.int32)
        tris = scene.tris_from_mesh(verts, labels)
        arrays = W.oracle_grid_arrays(W.oracle_grid(tris, solid["kind"] == "sphere", False))
        ids, counts, _ = W.host_walk(exe, d, arrays, tris, tris, W.KMAX, None, labels, labels)
        assert (counts == 0).all() and (ids == -1).all(), f"{solid['kind']}: {np.flatnonzero(counts)[:5]} touch a triangle that is no neighbour"
        matrix = scene.tri_tri_pairs(np.repeat(tris, nf, axis=0), np.tile(tris, (nf, 1))).reshape(nf, nf)
        glo, ghi = scene.grid_box(tris)
        boxes = scene.clip_boxes(scene.query_boxes(tris, glo, ghi), glo, ghi)
        matrix &= scene.overlap_pairs(np.tile(tris, (nf, 1)), np.repeat(boxes, nf, axis=0)).reshape(nf, nf)
        shares = (labels[:, None, :, None] == labels[None, :, None, :]).any(axis=(2, 3))
        assert (matrix >= shares).all(), "a triangle meets itself and every triangle it shares a vertex with"
        assert (matrix == shares).all(), "and, on a closed solid, no other"
        # without labels: the whole neighbourhood, paged
        got = np.zeros((nf, nf), dtype=bool)
        first = np.zeros(nf, dtype=np.int32); live = np.arange(nf)
        while live.size:
            ids, counts, _ = W.host_walk(exe, d, arrays, tris, tris[live], W.KMAX, first[live])
            assert not got[np.repeat(live, W.KMAX)[ids.reshape(-1) >= 0], ids[ids >= 0]].any()
            got[np.repeat(live, W.KMAX)[ids.reshape(-1) >= 0], ids[ids >= 0]] = True
            more = counts == W.KMAX + 1
            first[live[more]] = ids[more, W.KMAX - 1] + 1
            live = live[more]
        assert (got == matrix).all(), "without labels every triangle reports its neighbours"
        # every pair once
        once = np.zeros((nf, nf), dtype=np.int32)
        first = np.arange(1, nf + 1, dtype=np.int32); live = np.arange(nf)
        while live.size:
            ids, counts, _ = W.host_walk(exe, d, arrays, tris, tris[live], W.KMAX, first[live])
            np.add.at(once, (np.repeat(live, W.KMAX)[ids.reshape(-1) >= 0], ids[ids >= 0]), 1)
            more = counts == W.KMAX + 1
            first[live[more]] = ids[more, W.KMAX - 1] + 1
            live = live[more]
        assert (once == np.triu(matrix, 1)).all(), "first[i] = i + 1: every pair exactly once"


def test_host_program_under_the_sanitizers(fixture, scenes, tmp_path):
    """the host program, built stand-alone with address and undefined-behaviour sanitizers, runs the walk on the mesh queries clean: no index leaves the grid
    arrays, the labels or the id list; no float-to-int cast overflows"""
    exe = W.build_host(tmp_path, sanitize=True)
    tris, q, first, qlab, tlab = scenes["mesh"]
    arrays = W.oracle_grid_arrays(W.oracle_grid(tris, True, False))
    for k, any_ in ((W.KMAX, False), (1, True)):
        ids, counts, _ = W.host_walk(exe, tmp_path, arrays, tris, q, k, first, qlab, tlab, any_=any_)
        if not any_:
            W.assert_answers_equal(ids, counts, *W.expected(fixture, "mesh_lab", k), "the sanitized walk")
    ids, counts = W.host_brute(exe, tmp_path, tris, q[W.INACTIVE.start - 64:W.FLAT.start + 64], 3)
    assert (counts[64:64 + 96] == 0).all()


def test_header_library_and_bindings(fixture):
    from hagrid_amd import api, lib
    text = open(os.path.join(ROOT, "include", "hagrid_amd.h")).read()
    assert re.search(r"int\s+hagrid_overlap_tris\s*\(\s*hagrid_ctx\*\s*ctx,\s*const hagrid_grid\*\s*grid,\s*const void\*\s*tris,\s*const void\*\s*queries,\s*int num_queries,"
                     r"\s*const void\*\s*first,\s*const void\*\s*query_labels,\s*const void\*\s*tri_labels,\s*int k,\s*void\*\s*ids,\s*void\*\s*counts,\s*void\*\s*counters,"
                     r"\s*uint32_t flags\)", text)
    assert re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", text)
    assert "hagrid_overlap_tris" in lib.SIGNATURES and len(lib.SIGNATURES["hagrid_overlap_tris"][1]) == 13 and lib.ABI_VERSION == 3
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT hagrid_overlap_tris\b", exported)
    for name in ("overlap_tris", "self_intersections"):
        assert name in api.__all__ and callable(getattr(api, name))
    assert callable(api.MeshScene.vertex_labels) and callable(scene.overlap_tris) and callable(scene.tri_tri_pairs)
    shim = open(os.path.join(ROOT, "include", "hagrid", "traverse.h")).read()
    assert "overlap_tris" in shim
