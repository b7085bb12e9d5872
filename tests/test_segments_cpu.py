"""Capsule queries (hagrid_segment_tris), the part that needs no GPU: the numpy statement hagrid_amd/scene.py segment_tris, the header's brute force
(tests/cpp/segments_host.cpp) and the fixture tests/golden/segments.npz against each other, bit for bit; the host walk -- the walk the gfx950 kernel
runs -- over grids of the CPU oracle against the fixture for several k; every promise of hagrid_amd.h; paging to the end; the labelled answer on a
mesh's own edges; the deep grids of _deep_grids at every stage, once more under sanitizers; seg_tri against exact arithmetic; what the separating axes
prune; the kernel's resources and the kernel budget; the entry point in header, library and bindings."""
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
import _segments as SG
from hagrid_amd import scene

ROOT = K.ROOT
INC = K.INC


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return np.load(SG.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("segments_host")
    return SG.build_host(d), d


@pytest.fixture(scope="module")
def point_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("segments_point_host")
    return NK.build_host(d), d


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name in K.SCENES:
        tris = K.make_tris(name)
        tl, own = SG.fixture_labels(name, tris)
        out[name] = (tris, SG.fixture_segments(tris, name), SG.fixture_query_labels(own), tl)
    return out


_GRIDS = {}


def grid_arrays(scenes, name, compress, subset_only):
    key = (name, compress, subset_only)
    if key not in _GRIDS:
        _GRIDS[key] = K.oracle_grid_arrays(K.oracle_grid(scenes[name][0], compress, subset_only))
    return _GRIDS[key]


@pytest.mark.parametrize("name", K.SCENES)
def test_statement_host_brute_force_and_fixture_agree(fixture, scenes, host, name):
    """segments_host brute == the fixture (made by scene.segment_tris) for all 4096 segments at k = 8; scene.segment_tris again on a slice of every
    family (_segments.SAMPLE), entries and records; the stored pages; seg_tri pair by pair, numpy against the header"""
    exe, d = host
    tris, s, ql, tl = scenes[name]
    assert int(fixture[name + "_query_sum"]) == int(K.bits(s).astype(np.uint64).sum()), "the fixture's segments are the generators' segments"
    want, want_pages = SG.fixture_lists(fixture, name)
    be, br = SG.host_brute(exe, d, tris, s, SG.KMAX, query_labels=ql, tri_labels=tl)
    NK.assert_lists_equal(be, want, f"{name}: brute force of capsule.h against the fixture")
    plain = np.setdiff1d(np.arange(SG.NUM_SEGMENTS), np.arange(SG.OWN.start, SG.OWN.stop))[::5]
    NK.assert_lists_equal(SG.host_brute(exe, d, tris, s[plain], SG.KMAX)[0], want[plain], f"{name}: labels of -1 skip nothing")
    e, r = scene.segment_tris(tris, s[SG.SAMPLE], SG.KMAX, query_labels=ql[SG.SAMPLE], tri_labels=tl)
    NK.assert_lists_equal(e, want[SG.SAMPLE], f"{name}: scene.segment_tris against the fixture")
    NK.assert_lists_equal(br[SG.SAMPLE], r, f"{name}: records of the brute force against the statement")
    ss, sl = s[SG.STORED], ql[SG.STORED]
    got = NK.first_pages(lambda cursors: SG.host_brute(exe, d, tris, ss, SG.PAGE_K, cursors=cursors, query_labels=sl, tri_labels=tl)[0], ss.shape[0])
    NK.assert_lists_equal(got.reshape(-1, SG.PAGE_K), want_pages.reshape(-1, SG.PAGE_K), f"{name}: pages of the brute force against the fixture")
    # pair by pair: the winners of every list, their segment against their triangle
    qi, sj = np.nonzero(be["id"] >= 0)
    qi, sj = qi[::7], sj[::7]
    hp = SG.host_pairs(exe, d, tris[be["id"][qi, sj]], s[qi])
    sp = scene.segment_pairs(tris[be["id"][qi, sj]], s[qi])
    for key in ("valid", "d2", "q", "feature", "side", "s"):
        assert (np.ascontiguousarray(hp[key]).view(np.uint8) == np.ascontiguousarray(sp[key]).view(np.uint8)).all(), f"{name}: seg_tri {key}"
    assert (K.bits(hp["d2"]) == K.bits(be["d2"][qi, sj])).all()
    assert os.path.getsize(SG.FIXTURE) <= os.path.getsize(NK.FIXTURE), "no larger than nearest_k.npz"


def test_fixture_semantics(fixture, scenes, host):
    exe, d = host
    for name in K.SCENES:
        tris, s, ql, tl = scenes[name]
        e, _ = SG.fixture_lists(fixture, name)
        used = e["id"] >= 0
        own = e[SG.OWN]
        shares = ((tl[own["id"].clip(0)][:, :, :, None] == ql[SG.OWN][:, None, None, :]).any(axis=(2, 3))) & (own["id"] >= 0)
        assert not shares.any() and (own["id"] >= 0).any(axis=1).sum() > 128, "an own edge does not see the triangles that share a vertex with it"
        r2 = s[:, 3] * s[:, 3]
        assert (used[:, :-1] >= used[:, 1:]).all(), "used slots come first"
        d_ok = (e["d2"][:, :-1] < e["d2"][:, 1:]) | ((e["d2"][:, :-1] == e["d2"][:, 1:]) & (e["id"][:, :-1] < e["id"][:, 1:]))
        assert (d_ok | ~used[:, 1:]).all(), "sorted by (d2, id), no triangle twice"
        assert (e["d2"][used] <= np.broadcast_to(r2[:, None], e.shape)[used]).all()
        inactive = s[:, 3] < 0
        assert inactive.sum() == 16 and (e["id"][inactive] == -1).all() and (e["d2"][inactive] == -1).all()
        bad = ~np.isfinite(s[:, [0, 1, 2, 4, 5, 6]]).all(axis=1) | np.isnan(s[:, 3])
        assert bad.sum() == 8 + 8 + 8 + 8 and (e["id"][bad] == -1).all(), "NaN and infinite coordinates (the ZERO section's NaN points among them), NaN radii"
        rest = ~used & ~inactive[:, None]
        assert (K.bits(e["d2"])[rest] == np.broadcast_to(K.bits(r2)[:, None], e.shape)[rest]).all(), "an unused slot holds r2"
        assert 0 < used[SG.SHORT_R, 0].sum() and not used[SG.SHORT_R].all(axis=1).all()
        # the families are what they say: piercing segments find d2 = 0 with feature 4, segments on edges d2 = 0 ties decided by id
        _, r = SG.host_brute(exe, d, tris, s[SG.PIERCE], 1)
        assert ((r["feature"][:, 0] == 4) & (r["d2"][:, 0] == 0) & (r["s"][:, 0] > 0) & (r["s"][:, 0] < 1)).sum() > 200, name
        on = e[SG.EDGE][0::3]
        assert (on["d2"][:, 0] == 0).sum() > on.shape[0] // 2 and (((on["d2"][:, 0] == 0) & (on["d2"][:, 1] == 0) & (on["id"][:, 0] < on["id"][:, 1])).sum() > (8 if name == "mesh" else 0))


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", K.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, scenes, host, scene_name, compress, subset_only):
    """promises 1 and 2: entries bit-equal for all 4096 segments and k in {1, 2, 3, 5, 8} over Cell and SmallCell grids of the CPU oracle, both expansion
    modes: the list for k is the first k slots of the list for 8; the records are the brute force's"""
    exe, d = host
    tris, s, ql, tl = scenes[scene_name]
    arrays = grid_arrays(scenes, scene_name, compress, subset_only)
    want, _ = SG.fixture_lists(fixture, scene_name)
    trivial = (s[:, 3] < 0) | ~np.isfinite(s[:, [0, 1, 2, 4, 5, 6]]).all(axis=1) | np.isnan(s[:, 3])
    for k in (1, 2, 3, 5, 8):
        e, r, counts = SG.host_walk(exe, d, arrays, tris, s, k, query_labels=ql, tri_labels=tl)
        NK.assert_lists_equal(e, want[:, :k], f"{scene_name} compress={compress} subset_only={subset_only} k={k}")
        assert (r["id"] == e["id"]).all() and (K.bits(r["d2"]) == K.bits(e["d2"])).all()
        assert ((e["id"][:, k - 1] >= 0) == (counts[:, 3] != 0)).all()
        assert (counts[trivial] == 0).all() and (counts[~trivial, 0] >= 1).all()
    _, br = SG.host_brute(exe, d, tris, s[::16], 8, query_labels=ql[::16], tri_labels=tl)
    NK.assert_lists_equal(r[::16], br, f"{scene_name}: records of the walk against the brute force")
    unused = r["id"] < 0
    assert (K.bits(r["q"])[unused] == np.broadcast_to(K.bits(s[:, None, 0:3]), r["q"].shape)[unused]).all() and (K.bits(r["s"])[unused] == 0).all()
    assert (r["feature"][unused] == 0).all() and (r["side"][unused] == 0).all()
    if not compress and subset_only:
        print(scene_name, "triangles tested per query at k = 8:", counts[:, 1].mean())


@pytest.mark.parametrize("scene_name", K.SCENES)
def test_zero_length_is_the_point_query(fixture, scenes, host, point_host, scene_name):
    """promise 5: a == b with the first label of each pair (second -1): entries and records are hagrid_nearest_tris' for the points (a, r) -- the host walk
    of closest.h -- bit for bit, labelled and unlabelled; at k = 1 without cursor or labels the records are tests/golden/closest.npz"""
    exe, d = host
    pexe, pd = point_host
    tris, s = scenes[scene_name][:2]
    arrays = grid_arrays(scenes, scene_name, True, True)
    z = s[SG.ZERO]
    assert (K.bits(z[:, 0:3]) == K.bits(z[:, 4:7])).all()
    pts = np.ascontiguousarray(z[:, 0:4])
    rng = np.random.default_rng(3)
    tl = rng.integers(0, 64, (tris.shape[0], 3)).astype(np.int32)
    ql = rng.integers(-1, 64, z.shape[0]).astype(np.int32)
    ql2 = np.stack([ql, np.full_like(ql, -1)], axis=1)
    for k in (1, 8):
        for labelled in (False, True):
            e, r, _ = SG.host_walk(exe, d, arrays, tris, z, k, query_labels=ql2 if labelled else None, tri_labels=tl if labelled else None)
            pe, pr, _ = NK.host_walk(pexe, pd, arrays, tris, pts, k, query_labels=ql if labelled else None, tri_labels=tl if labelled else None)
            NK.assert_lists_equal(e, pe, f"{scene_name} k={k} labelled={labelled}: entries against the point query")
            NK.assert_lists_equal(r.view(scene.CLOSEST_DTYPE), pr, f"{scene_name} k={k} labelled={labelled}: records against the point query")
    want = K.fixture_results(np.load(K.FIXTURE), scene_name)[SG.ZERO_POINTS]
    e, r, _ = SG.host_walk(exe, d, arrays, tris, z, 1)
    K.assert_results_equal(r[:, 0].view(scene.CLOSEST_DTYPE), want, f"{scene_name}: k = 1 against the nearest-surface fixture")
    # the pair function itself: seg_tri with a == b is point_tri, s = +0
    t = tris[:z.shape[0]]
    sp, cp = scene.segment_pairs(t, z), scene.closest_pairs(t, pts)
    ok = np.isfinite(pts[:, 0:3]).all(axis=1)
    for key in ("d2", "q", "feature", "side"):
        assert (np.ascontiguousarray(sp[key][ok]).view(np.uint8) == np.ascontiguousarray(cp[key][ok]).view(np.uint8)).all(), key
    assert (K.bits(sp["s"]) == 0).all()


# the segments that must page, counted with the numpy statement: (two or more pages, four or more)
MUST_PAGE = {"soup": (500, 300), "mesh": (500, 300)}


@pytest.mark.parametrize("scene_name", K.SCENES)
def test_paging_to_the_end(fixture, scenes, host, scene_name):
    """promise 3: k = 3, every segment with a finite radius (_segments.PAGED) paged to its end over a SmallCell grid: the concatenation is
    scene.tris_near_segments; the first three pages are the fixture's"""
    exe, d = host
    tris, s, ql, tl = scenes[scene_name]
    arrays = grid_arrays(scenes, scene_name, True, True)
    ss, sl = s[SG.PAGED], ql[SG.PAGED]
    lists, pages = NK.page_through(lambda which, cursors: SG.host_walk(exe, d, arrays, tris, ss[which], SG.PAGE_K, cursors=cursors, query_labels=sl[which],
                                                                       tri_labels=tl)[0], ss.shape[0], SG.PAGE_K, max_pages=256)
    csr = scene.tris_near_segments(tris, ss, query_labels=sl, tri_labels=tl)
    NK.assert_pages_equal_csr(lists, csr, scene_name)
    sizes = np.diff(csr["offsets"])
    print(scene_name, "segments with >= 3 candidates:", int((sizes >= 3).sum()), ">= 9:", int((sizes >= 9).sum()), "longest:", int(sizes.max()))
    assert (pages == sizes // SG.PAGE_K + 1).all()
    two, four = MUST_PAGE[scene_name]
    assert (pages >= 2).sum() >= two and (pages >= 4).sum() >= four, "the lists must page"
    assert (pages[-256:] >= 2).sum() >= 64, "the labelled lists page as well"
    _, want_pages = SG.fixture_lists(fixture, scene_name)
    got = NK.first_pages(lambda cursors: SG.host_walk(exe, d, arrays, tris, ss, SG.PAGE_K, cursors=cursors, query_labels=sl, tri_labels=tl)[0], ss.shape[0])
    NK.assert_lists_equal(got.reshape(-1, SG.PAGE_K), want_pages.reshape(-1, SG.PAGE_K), f"{scene_name}: pages of the walk against the fixture")
    # a cursor of d2 = -1 excludes nothing, a cursor with a NaN d2 everything
    n = ss.shape[0]
    want8 = SG.fixture_lists(fixture, scene_name)[0][SG.STORED]
    cur = NK.entries_of(np.full(n, -1.0, np.float32), np.full(n, 2 ** 31 - 1, np.int32))
    NK.assert_lists_equal(SG.host_walk(exe, d, arrays, tris, ss, 8, cursors=cur, query_labels=sl, tri_labels=tl)[0], want8, "cursor (-1, INT_MAX)")
    cur = NK.entries_of(np.full(n, np.nan, np.float32), np.full(n, -1, np.int32))
    e = SG.host_walk(exe, d, arrays, tris, ss, 8, cursors=cur)[0]
    assert (e["id"] == -1).all() and (K.bits(e["d2"]) == K.bits(ss[:, 3] * ss[:, 3])[:, None]).all()


def test_labels_on_the_meshs_own_edges(host):
    """promise 4: the stadium mesh, its own edges as segments with their two vertex indices as labels and the index triples as triangle labels: the walk
    is the brute force and, on a slice, the numpy statement; no list holds a triangle that shares a vertex with the edge; it is the unlabelled
    statement over the scene without those triangles; without labels the first entries ARE the triangles of the edge at d2 = 0; labels of -1 skip nothing"""
    exe, d = host
    tris, F, s, labels = SG.edge_labels_case()
    arrays = K.oracle_grid_arrays(K.oracle_grid(tris, True, True))
    k = 8
    e, r, _ = SG.host_walk(exe, d, arrays, tris, s, k, query_labels=labels, tri_labels=F)
    be, br = SG.host_brute(exe, d, tris, s, k, query_labels=labels, tri_labels=F)
    want = be
    NK.assert_lists_equal(e, be, "labelled walk against the labelled brute force")
    NK.assert_lists_equal(r, br, "labelled walk against the brute force: records")
    pick = np.arange(0, s.shape[0], max(1, s.shape[0] // 64))
    se, sr = scene.segment_tris(tris, s[pick], k, query_labels=labels[pick], tri_labels=F)
    NK.assert_lists_equal(se, want[pick], "the statement on a slice")
    NK.assert_lists_equal(sr, r[pick], "the statement on a slice: records")
    shares = ((F[e["id"].clip(0)][:, :, :, None] == labels[:, None, None, :]).any(axis=(2, 3))) & (e["id"] >= 0)
    assert not shares.any(), "a list holds a triangle that shares a vertex with the edge"
    assert (e["id"] >= 0).any(axis=1).sum() > s.shape[0] // 2, "most edges have neighbours they share no vertex with"
    # the scene with the skipped triangles removed (their stored normal cleared: no surface, ids unchanged), a slice of the edges
    for i in pick[:48]:
        t2 = tris.copy()
        gone = (F[:, :, None] == labels[i][None, None, :]).any(axis=(1, 2))
        t2[gone] = t2[gone] * np.float32([1, 1, 1, 0] * 3)
        NK.assert_lists_equal(SG.host_brute(exe, d, t2, s[i:i + 1], k)[0], e[i:i + 1], f"edge {i}: the unlabelled answer without its triangles")
    plain, _, _ = SG.host_walk(exe, d, arrays, tris, s, k)
    minus, _, _ = SG.host_walk(exe, d, arrays, tris, s, k, query_labels=np.full((s.shape[0], 2), -1, np.int32), tri_labels=F)
    NK.assert_lists_equal(minus, plain, "labels of -1 skip nothing")
    own = ((F[plain["id"].clip(0)][:, :, :, None] == labels[:, None, None, :]).any(axis=(2, 3))) & (plain["id"] >= 0)
    # (an edge may also touch triangles it shares no vertex with -- the floor under a pillar -- and a smaller id wins the tie at d2 = 0)
    assert own[:, 0].mean() > 0.5 and own.any(axis=1).mean() > 0.9 and (plain["id"] != e["id"]).any(), "without labels an edge finds the triangles around it"
    one, _, _ = SG.host_walk(exe, d, arrays, tris, s, k, query_labels=np.stack([labels[:, 0], np.full(s.shape[0], -1, np.int32)], axis=1), tri_labels=F)
    assert (one["id"] != e["id"]).any() and (one["id"] != plain["id"]).any(), "each of the two labels skips on its own"


@pytest.fixture(scope="module")
def deep_hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("segments_deep")
    return {"plain": SG.build_host(d), "san": SG.build_host(d, sanitize=True), "dir": d}


def deep_segments(tris):
    """the points of _deep_grids as segments: each point to the next one but 17 (long ones across the scene), every fourth of no length"""
    p = D.points(tris)
    s = scene.make_segments(p[:, 0:3], np.roll(p[:, 0:3], 17, axis=0), p[:, 3])
    s[0::4, 4:7] = s[0::4, 0:3]
    s[1::4, 4:7] = s[1::4, 0:3] + (s[1::4, 4:7] - s[1::4, 0:3]) * np.float32(0.01)
    return s


@pytest.mark.parametrize("name", D.WALKED)
def test_deep_grids_at_every_stage(deep_hosts, name):
    """every scene and stage of _deep_grids.CATALOGUE: the host walk at k = 8 against the host brute force, bit for bit; once more with the stand-alone
    sanitizer build of the host program (-fsanitize=address,undefined, run directly)"""
    d = deep_hosts["dir"]
    tris = D.make_tris(name)
    s = deep_segments(tris)
    want_e, want_r = SG.host_brute(deep_hosts["plain"], d, tris, s, 8)
    assert ((want_e["id"] >= 0).sum(axis=1) >= 2).sum() > s.shape[0] // 4
    st = D.OracleStages(name, tris)
    for stage in D.stages_of(name):
        out = D.stage_grid(st, stage)
        G = out[0] if stage == "compress" else out
        arrays = _host.oracle_grid_arrays(G)
        for which in ("plain", "san"):
            e, r, _ = SG.host_walk(deep_hosts[which], d, arrays, tris, s, 8)
            NK.assert_lists_equal(e, want_e, f"{name} after {stage} ({which})")
            NK.assert_lists_equal(r, want_r, f"{name} after {stage} ({which}): records")


def test_sanitizer_build_on_the_fixture_scene(fixture, scenes, deep_hosts):
    """the stand-alone sanitizer build once more, on the soup: the modes pairs, brute and walk, with labels (the OWN section and a slice of every other
    one) and cursors (the second page at k = 3): the plain build's bits, which the other tests hold to the fixture"""
    d = deep_hosts["dir"]
    tris, s, ql, tl = scenes["soup"]
    pick = np.unique(np.concatenate([np.arange(0, SG.NUM_SEGMENTS, 32), np.arange(SG.OWN.start, SG.OWN.stop, 4), np.arange(SG.SPECIAL.start, SG.SPECIAL.stop)]))
    ss, sl = s[pick], ql[pick]
    arrays = grid_arrays(scenes, "soup", True, True)
    want, _ = SG.fixture_lists(fixture, "soup")
    out = {}
    for which in ("plain", "san"):
        exe = deep_hosts[which]
        be, br = SG.host_brute(exe, d, tris, ss, SG.PAGE_K, query_labels=sl, tri_labels=tl)
        cur = np.ascontiguousarray(be[:, -1]); cur[be["id"][:, -1] < 0] = (-1.0, -1)
        be2, br2 = SG.host_brute(exe, d, tris, ss, SG.PAGE_K, cursors=cur, query_labels=sl, tri_labels=tl)
        we2, wr2, wc = SG.host_walk(exe, d, arrays, tris, ss, SG.PAGE_K, cursors=cur, query_labels=sl, tri_labels=tl)
        hp = SG.host_pairs(exe, d, tris[be["id"][:, 0].clip(0)], ss)
        out[which] = (be, br, be2, br2, we2, wr2, wc, np.stack([np.ascontiguousarray(hp[k]).view(np.uint32).reshape(len(pick), -1).astype(np.uint32) for k in ("d2", "q", "feature", "side", "s")][:1]))
        NK.assert_lists_equal(be, want[pick][:, :SG.PAGE_K], f"{which}: the first page against the fixture")
        NK.assert_lists_equal(we2, be2, f"{which}: the second page, walk against brute force")
        NK.assert_lists_equal(wr2, br2, f"{which}: the second page, records")
        full = be["id"][:, -1] >= 0                              # the others kept the cursor (-1, -1) and answer the same again
        assert full.sum() > 64 and (be2["id"][full] >= 0).any() and (be2["id"][full][:, :1] != be["id"][full]).all()
        NK.assert_lists_equal(be2[~full], be[~full], f"{which}: a list that was not full, asked again")
    for a, b in zip(out["plain"], out["san"]):
        assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all(), "the sanitizer build gives other bits"


def test_seg_tri_against_exact_arithmetic():
    """500 pairs on integer coordinates |c| <= 64 (_segments.exact_family: crossing, touching at a vertex, parallel to an edge, coplanar, skew), seg_tri's
    d2 against the distance in rationals (fractions.Fraction, written independently: _segments.exact_seg_tri).  The error of a pair is
    |d2 - exact| / max(exact, 1): relative, and absolute in lattice units below one.  The bar is 4 x point_tri's largest error against ITS rational
    value on the same family's ends (seg_tri's chain holds two divisions and a clamp more).  Measured: point_tri 1.40e-6, so the bar is 5.6e-6;
    seg_tri 1.88e-6 (a parallel pair); every crossing and touching pair gives exactly 0."""
    v0, v1, v2, a, b = SG.exact_family()
    n = a.shape[0]
    tris = scene.tris_from_vertices(v0.astype(np.float32), v1.astype(np.float32), v2.astype(np.float32))
    got = scene.segment_pairs(tris, scene.make_segments(a, b, np.inf))
    pa, pb = scene.closest_pairs(tris, a.astype(np.float32)), scene.closest_pairs(tris, b.astype(np.float32))
    assert got["valid"].all()

    def err(f, x):
        return abs(float(f) - float(x)) / max(float(x), 1.0)

    e_seg, e_pt, exact = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        V = [SG._F3(v) for v in (v0[i], v1[i], v2[i])]
        A, B = SG._F3(a[i]), SG._F3(b[i])
        x = SG.exact_seg_tri(A, B, *V)
        exact[i] = float(x)
        e_seg[i] = err(got["d2"][i], x)
        e_pt[i] = max(err(pa["d2"][i], SG.exact_point_tri(A, *V)), err(pb["d2"][i], SG.exact_point_tri(B, *V)))
    per = n // 5
    print("point_tri's largest error:", e_pt.max(), " seg_tri's:", e_seg.max(), " by class:", [float(e_seg[c * per:(c + 1) * per].max()) for c in range(5)])
    assert (exact[:2 * per] == 0).all() and (exact[2 * per:] > 0).sum() > per, "the crossing and touching classes touch; the others mostly do not"
    assert (got["feature"][:per] == 4).all() and (got["d2"][:2 * per] == 0).all()
    assert 0 < e_pt.max() < 1e-5
    assert e_seg.max() <= 4 * e_pt.max()


@pytest.mark.parametrize("scene_name", K.SCENES)
def test_the_separating_axes_prune(scenes, host, scene_name):
    """over the long-diagonal family the host walk tests, on average, fewer than half of the scene's triangles per query; with the box-to-box bound alone
    it tests more than all of them (the segment's box is the scene; a triangle is offered once per cell that references it).  Measured at k = 8,
    triangles tested per query: soup (20 000 triangles) 624 with the axes, 151 977 without; mesh (3 356) 158 against 28 199."""
    exe, d = host
    tris, s = scenes[scene_name][:2]
    arrays = grid_arrays(scenes, scene_name, True, True)
    e, _, counts = SG.host_walk(exe, d, arrays, tris, s[SG.LONG], 8)
    eb, _, box = SG.host_walk(exe, d, arrays, tris, s[SG.LONG], 8, box_only=True)
    NK.assert_lists_equal(e, eb, "the same answer with and without the axes")
    print(scene_name, "long diagonals, triangles tested per query:", counts[:, 1].mean(), "box only:", box[:, 1].mean(), "of", tris.shape[0])
    assert counts[:, 1].mean() < tris.shape[0] / 2
    assert box[:, 1].mean() > tris.shape[0]


def test_kernel_resources_and_budget(fixture):
    """tools/kernel_resources.py: capsule.hip holds segment_tris_kernel alone, at most 128 VGPRs, no spill, no scratch, at least 4 wavefronts per SIMD;
    closest.hip is as test_nearest_k_cpu reads it and as the parent commit built it: two kernels, closest_points_kernel at 94 VGPRs and 5 wavefronts,
    nearest_tris_kernel at 103 VGPRs; frame.hip, whose two kernels became one to pay for the new one, holds frame_kernel alone without scratch; at most
    120 kernels"""
    rows = _host.kernel_rows("capsule")
    assert set(rows) == {"segment_tris_kernel"}, rows
    vgpr, spill, scratch, occ = rows["segment_tris_kernel"]
    assert vgpr <= 128 and spill == 0 and scratch == 0 and occ >= 4, rows
    rows = _host.kernel_rows("closest")
    assert set(rows) == {"closest_points_kernel", "nearest_tris_kernel"}, rows
    assert rows["closest_points_kernel"] == (94, 0, 0, 5) and rows["nearest_tris_kernel"] == (103, 0, 0, 4), rows
    rows = _host.kernel_rows("frame")
    assert set(rows) == {"frame_kernel"} and rows["frame_kernel"][1:3] == (0, 0), rows
    c = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "count_kernels.py")], capture_output=True, text=True, cwd=ROOT)
    m = re.search(r"(\d+) kernels", c.stdout)
    assert m and int(m.group(1)) <= 120, c.stdout[-300:] + c.stderr[-300:]


def test_records_and_entry_point(fixture):
    """the ctypes mirror: record sizes and offsets, the symbol declared in the header, exported by the library and bound"""
    from hagrid_amd import api, lib
    S, R = scene.SEGMENT_DTYPE, scene.SEGMENT_RECORD_DTYPE
    assert S.itemsize == 32 and [S.fields[k][1] for k in ("a", "r", "b", "pad")] == [0, 12, 16, 28]
    assert R.itemsize == 32 and [R.fields[k][1] for k in ("q", "d2", "id", "feature", "side", "s")] == [0, 12, 16, 20, 24, 28]
    assert [R.fields[k][1] for k in ("q", "d2", "id", "feature", "side")] == [scene.CLOSEST_DTYPE.fields[k][1] for k in ("q", "d2", "id", "feature", "side")]
    assert api.SEGMENT_DTYPE is S and api.SEGMENT_RECORD_DTYPE is R
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "hagrid_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+hagrid_segment_tris\s*\(", code) and re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", code)
    L = lib.load()
    assert "hagrid_segment_tris" in lib.SIGNATURES and hasattr(L, "hagrid_segment_tris") and len(lib.SIGNATURES["hagrid_segment_tris"][1]) == 13
    assert L.hagrid_abi_version() == 3
    for name in ("segment_tris", "tris_near_segments", "SEGMENT_DTYPE", "SEGMENT_RECORD_DTYPE"):
        assert hasattr(api, name) and name in api.__all__
    assert hasattr(api.MeshScene, "edge_labels")
    for name in ("segment_pairs", "segment_tris", "tris_near_segments", "make_segments_short", "make_segments_diagonal", "make_segments_axis",
                 "make_segments_on_edges", "make_segments_piercing", "make_segments_outside", "mesh_edges"):
        assert hasattr(scene, name)
    prog = '#include "hagrid_amd.h"\nint main(void) { return sizeof(&hagrid_segment_tris) ? 0 : 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-fsyntax-only", "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
