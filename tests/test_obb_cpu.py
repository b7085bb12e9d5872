"""Oriented-box queries (hagrid_overlap_obbs), the part that needs no GPU.  The yardstick of the pair is exact arithmetic (tests/_obb.py exact_meet, stored by
tests/golden/make_golden_obb.py in tests/golden/obb.npz): obb_meets of include/hagrid/obb.h (compiled for the host) and scene.obb_pairs on half-integer
pairs, where float32 is exact; axis-aligned records against the box query; the host walk tests/cpp/obb_host.cpp -- the walk the gfx950 kernel runs -- over
grids of the CPU oracle against the host brute force, the numpy statement and the fixture, for k = 1, 2, 3, 5, 8 and ANY, both cell formats and both
expansion modes; paging; labels; the deep grids at every stage; what the float prune saves on thin diagonal planks; rounding on scene pairs; the host
program under the sanitizers; the kernel's resources, the kernel count, the entry point in header, library and bindings."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _deep_grids as D
import _host
import _obb as B
import _overlap as V
from hagrid_amd import scene

ROOT = B.ROOT


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return np.load(B.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("obb_host")
    return B.build_host(d), d


@pytest.fixture(scope="module")
def scenes(fixture):
    """name -> (tris, records, query_labels, tri_labels)"""
    out = {}
    for name in B.SCENES:
        tris = B.make_tris(name)
        out[name] = (tris, *B.scene_queries(fixture, name, tris), B.scene_labels(tris.shape[0]))
    return out


def members(tris, q, ids, query_labels=None, tri_labels=None):
    """is ids[i] (>= 0) a member of S_i, by the numpy statement of every condition?"""
    glo, ghi = scene.grid_box(tris)
    boxes = scene.clip_boxes(scene.obb_boxes(q, glo, ghi), glo, ghi)
    ok = scene.overlap_pairs(tris[ids], boxes) & scene.obb_pairs(tris[ids], q) & scene.tris_have_surface(tris[ids]) & (ids >= q["first"])
    if query_labels is not None:
        ok &= ~((query_labels >= 0)[:, None] & (query_labels[:, None] == tri_labels[ids])).any(axis=1)
    return ok


def test_lattice_pairs_equal_the_exact_test(fixture, host):
    """(a): obb_meets through the host program and scene.obb_pairs equal the exact truth on all 16 384 pairs on half-integer coordinates within the bound
    the header states, pair by pair -- rotations by multiples of 90 degrees, integer frames, sheared frames; an eighth touch at a face, an edge or a vertex"""
    exe, d = host
    obbs, tris, P = B.lattice_pairs()
    assert tris.shape[0] == B.NUM_LATTICE_PAIRS >= 16384 and B.array_sum(obbs) + B.array_sum(tris) == int(fixture["lattice_pair_sum"])
    O = scene._obb_rows(obbs)
    assert np.abs(scene.tri_vertices(tris)).max() <= 16 and np.abs(O[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]).max() <= 16, "the bound of obb.h"
    assert (np.abs(P) % 2 == 1).any(), "half-integers occur"
    truth = np.unpackbits(fixture["lattice_truth"])[:B.NUM_LATTICE_PAIRS].astype(bool)
    got = scene.obb_pairs(tris, obbs)
    assert (got == truth).all(), f"scene.obb_pairs: {(got != truth).sum()} of {truth.size} pairs differ from the exact test, first at {np.flatnonzero(got != truth)[:5]}"
    got = B.host_pairs(exe, d, obbs, tris)
    assert (got == truth).all(), f"obb_meets: {(got != truth).sum()} of {truth.size} pairs differ from the exact test, first at {np.flatnonzero(got != truth)[:5]}"
    t8 = B.NUM_LATTICE_PAIRS // 8
    assert truth[:t8].all(), "the touching eighth meets"
    for kind in range(3):                       # every family of frames says both
        sel = np.arange(t8, B.NUM_LATTICE_PAIRS)[np.arange(t8, B.NUM_LATTICE_PAIRS) % 3 == kind]
        assert truth[sel].sum() > 200 and (~truth[sel]).sum() > 200
    # the spot check of the yardstick itself: a few pairs again, now
    again = np.r_[0:24, t8:t8 + 40]
    assert (B.lattice_truth(P[again]) == truth[again]).all()


def test_axis_aligned_records_equal_the_box_query(fixture, host, tmp_path):
    """on the integer lattice scene, axis-aligned records whose bounds lie on half-integers (nothing touches) list what overlap::brute_force lists for the
    same boxes, k = 1, 3, 8 -- through the header's brute force, the walk and the numpy statement"""
    exe, d = host
    box_exe = V.build_host(tmp_path)
    tris, rec, boxes = B.lattice_scene()
    assert B.array_sum(tris) + B.array_sum(rec) == int(fixture["lattice_scene_sum"])
    assert ((boxes[:, [0, 1, 2, 4, 5, 6]] * 2) % 2 == 1).all(), "every bound on a half-integer"
    arrays = B.oracle_grid_arrays(B.oracle_grid(tris, False, False))
    sizes = fixture["lattice_sizes"]
    assert (sizes > B.KMAX + 1).any() and sizes.min() < sizes.max() // 4, "lists of many lengths"
    for k in (1, 3, 8):
        want = V.host_brute(box_exe, tmp_path, tris, boxes, k)
        B.assert_answers_equal(*want, *B.expected(fixture, "lattice", k), f"lattice scene k={k}: the fixture is the box query's brute force")
        B.assert_answers_equal(*B.host_brute(exe, d, tris, rec, k), *want, f"lattice scene k={k}: obb_brute_force")
        ids, counts, _ = B.host_walk(exe, d, arrays, tris, rec, k)
        B.assert_answers_equal(ids, counts, *want, f"lattice scene k={k}: the walk")
    r = scene.overlap_obbs(tris, rec, k=B.KMAX)
    B.assert_answers_equal(r["ids"], r["counts"], *B.expected(fixture, "lattice", B.KMAX), "lattice scene: scene.overlap_obbs")
    assert (r["sizes"] == sizes).all()


def test_fixture_is_the_statement_and_the_brute_force(fixture, scenes, host):
    """the stored answers are what the header's brute force gives on all queries (k = 8 and k = 1, with and without labels) and what scene.overlap_obbs
    gives on every 16th"""
    exe, d = host
    for name in B.SCENES:
        tris, q, qlab, tlab = scenes[name]
        for key, labels in ((name, (None, None)), (name + "_lab", (qlab, tlab))):
            for k in (B.KMAX, 1):
                ids, counts = B.host_brute(exe, d, tris, q, k, *labels)
                B.assert_answers_equal(ids, counts, *B.expected(fixture, key, k), f"{key} k={k}: the brute force")
            sub = slice(0, None, 16)
            r = scene.overlap_obbs(tris, q[sub], k=B.KMAX, query_labels=None if labels[0] is None else labels[0][sub], tri_labels=labels[1])
            want = B.expected(fixture, key, B.KMAX)
            B.assert_answers_equal(r["ids"], r["counts"], want[0][sub], want[1][sub], f"{key}: scene.overlap_obbs")
            assert (r["sizes"] == fixture[key + "_sizes"][sub]).all()


def test_fixture_semantics(fixture, scenes):
    for name in B.SCENES:
        tris, q, qlab, tlab = scenes[name]
        for key in (name, name + "_lab"):
            ids, sizes = fixture[key + "_ids"], fixture[key + "_sizes"]
            listed = ids >= 0
            assert (listed.sum(axis=1) == np.minimum(sizes, B.KMAX)).all(), "min(k, m) slots are used"
            assert (listed[:, :-1] >= listed[:, 1:]).all(), "the unused slots are the last ones"
            both = listed[:, :-1] & listed[:, 1:]
            assert (ids[:, 1:][both] > ids[:, :-1][both]).all() and ids.max() < tris.shape[0], "ascending, each id once"
            for k in B.KS:
                assert (sizes < k).any() and (sizes == k).any() and (sizes == k + 1).any() and (sizes > k + 1).any(), (key, k)
        sizes = fixture[name + "_sizes"]
        rows = scene._obb_rows(q)
        finite = np.isfinite(rows[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]).all(axis=1)
        assert (~finite).sum() == 64 and (~finite[B.BAD]).sum() == 64 and (sizes[~finite] == 0).all() and (fixture[name + "_ids"][~finite] == -1).all(), "NaN and inf: inactive"
        assert (sizes[B.BAD][2::4] > 0).any() and (sizes[B.BAD][3::4] > 0).any(), "huge axes are legal"
        assert (sizes[B.SMALL] > 0).sum() > 500 and (sizes[B.PLANK] > B.KMAX + 1).sum() >= 100 and (sizes[B.SHEAR] > 0).sum() > 50 and (sizes[B.FLAT] > 0).sum() > 50
        assert (sizes[B.OUTSIDE][3::4] == 0).all() and (sizes[B.OUTSIDE] > 0).any(), "wholly outside: nothing; partly outside: something"
        assert (sizes[B.FAR][0::2] == 0).all() and (sizes[B.FAR][1::2] > 0).sum() >= 32, "far centres: nothing, but where a long axis reaches back into the scene"
        eps = np.float32(max(np.abs(np.concatenate(scene.grid_box(tris))).max(), 0)) * np.float32(1.52587890625e-05)
        assert (np.abs(rows[B.FAR, 0:3]).max(axis=1) > eps * np.float32(262144.0)).all(), "the FAR centres lie beyond 4 M: the float prune is off for them"
        plain, lab = fixture[name + "_sizes"], fixture[name + "_lab_sizes"]
        assert (plain[B.OWN] >= 1).all(), "without labels the oriented box of a triangle finds the triangle"
        assert (lab[B.OWN] < plain[B.OWN]).all() and (np.delete(lab, np.r_[B.OWN]) == np.delete(plain, np.r_[B.OWN])).all(), "a body's box does not see the body"
        own_ids = fixture[name + "_lab_ids"][B.OWN]
        assert ((own_ids // B.BODY != qlab[B.OWN, None]) | (own_ids < 0)).all()
        src = fixture[name + "_ids"][B.PAGED_FROM:B.PAGED_FROM + 128]
        assert (q["first"][B.PAGED] == src[:, 2] + 1).all() and (q["first"][B.PAGED] > 0).sum() >= 64 and (q["first"][:B.PAGED.start] == 0).all()
        full = src[:, 2] >= 0
        assert (fixture[name + "_ids"][B.PAGED][full, :5] == src[full, 3:]).all(), "the page after the third id starts with the fourth"


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", B.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, scenes, host, scene_name, compress, subset_only):
    """ids and counts of all 4096 queries for k = 1, 2, 3, 5, 8 over Cell and SmallCell grids of the CPU oracle, both expansion modes, with labels and
    without; the prefix property; ANY; inactive queries take no walk"""
    exe, d = host
    tris, q, qlab, tlab = scenes[scene_name]
    G = B.oracle_grid(tris, compress, subset_only)
    assert (G.small_cells is not None) == compress
    arrays = B.oracle_grid_arrays(G)
    what = f"{scene_name} compress={compress} subset_only={subset_only}"
    rows = scene._obb_rows(q)
    inactive = ~np.isfinite(rows[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]).all(axis=1)
    prev = None
    for k in B.KS:
        ids, counts, totals = B.host_walk(exe, d, arrays, tris, q, k, qlab, tlab)
        B.assert_answers_equal(ids, counts, *B.expected(fixture, scene_name + "_lab", k), f"{what} k={k} with labels")
        assert (totals[inactive] == 0).all() and (totals[B.FAR][0::2, 1] == 0).all()
        if prev is not None:
            assert (ids[:, :prev.shape[1]] == prev).all(), "the prefix property"
        prev = ids
    for k in (B.KMAX, 2):
        ids, counts, _ = B.host_walk(exe, d, arrays, tris, q, k)
        B.assert_answers_equal(ids, counts, *B.expected(fixture, scene_name, k), f"{what} k={k} without labels")
    for key, labels in ((scene_name, (None, None)), (scene_name + "_lab", (qlab, tlab))):
        ids, counts, totals = B.host_walk(exe, d, arrays, tris, q, 1, *labels, any_=True)
        sizes = fixture[key + "_sizes"]
        assert ((ids[:, 0] >= 0) == (sizes > 0)).all() and (counts == (sizes > 0)).all() and (ids[sizes == 0, 0] == -1).all()
        hit = ids[:, 0] >= 0
        lab = (None, None) if labels[0] is None else (qlab[hit], tlab)
        assert members(tris, q[hit], ids[hit, 0], *lab).all(), "ANY returns a member of S"


@pytest.mark.parametrize("scene_name", B.SCENES)
def test_paging_reproduces_the_whole_list(scenes, host, scene_name):
    """a SAMPLE of each scene -- 64 BIG, 16 PLANK and 64 FLAT queries, not every query of the fixture: every list among them with more than 3 members, asked
    with k = 3 and first = last id + 1 again and again, is the whole brute-force set in order"""
    exe, d = host
    tris, q, _, _ = scenes[scene_name]
    pick = np.concatenate([np.arange(B.BIG.start, B.BIG.start + 64), np.arange(B.PLANK.start, B.PLANK.start + 16), np.arange(B.FLAT.start, B.FLAT.start + 64)])
    whole = scene.overlap_obbs(tris, q[pick], k=1 << 14)
    pick = pick[whole["sizes"] > 3]; ids_all = whole["ids"][whole["sizes"] > 3]; sizes = whole["sizes"][whole["sizes"] > 3]
    assert pick.size >= 64 and sizes.max() > 100
    qq = q[pick].copy()
    n = qq.shape[0]
    arrays = B.oracle_grid_arrays(B.oracle_grid(tris, True, False))
    pages = [[] for _ in range(n)]
    live = np.arange(n)
    for _ in range(int(sizes.max()) // 3 + 2):
        ids, counts, _ = B.host_walk(exe, d, arrays, tris, qq[live], 3)
        for row, i in enumerate(live):
            pages[i] += [int(v) for v in ids[row] if v >= 0]
        more = counts == 4
        assert (counts[~more] == (ids[~more] >= 0).sum(axis=1)).all()
        qq["first"][live[more]] = ids[more, 2] + 1
        live = live[more]
        if live.size == 0:
            break
    assert live.size == 0
    for i in range(n):
        assert pages[i] == [int(v) for v in ids_all[i, :sizes[i]]], f"query {pick[i]}"


def test_labels_are_the_scene_without_the_skipped_triangles(scenes, host):
    """the labelled answer of an OWN query is the unlabelled answer over the scene without the triangles of its body -- here: with those triangles made
    surfaceless (stored normal 0), which keeps the ids and the grid box"""
    exe, d = host
    tris, q, qlab, tlab = scenes["soup"]
    arrays = B.oracle_grid_arrays(B.oracle_grid(tris, False, False))
    pick = np.arange(B.OWN.start, B.OWN.start + 48)
    ids, counts, _ = B.host_walk(exe, d, arrays, tris, q[pick], B.KMAX, qlab[pick], tlab)
    for row, i in enumerate(pick):
        without = tris.copy()
        body = tlab[:, 0] == qlab[i]
        without[body, 3] = 0; without[body, 7] = 0; without[body, 11] = 0
        want = B.host_brute(exe, d, without, q[i:i + 1], B.KMAX, grid=scene.grid_box(tris))
        B.assert_answers_equal(ids[row:row + 1], counts[row:row + 1], *want, f"query {i}")


@pytest.mark.parametrize("name", D.WALKED)
def test_deep_grids_at_every_stage(host, name):
    """the deep grids of tests/_deep_grids.py after build, merge, flatten, expand and compress: the walk equals the brute force, with the prune and without"""
    exe, d = host
    tris = D.make_tris(name)
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    c = np.concatenate([V.vertices_of(tris[1500 if name == "nested" else 0:], 192, B.SEED + 50), scene.make_points_uniform(lo, hi, 64, B.SEED + 51)])
    half = (np.float32([1e-5, 1e-4, 1e-3, 5e-2])[np.arange(256) % 4][:, None] * (np.float32(0.5) + B._u(B.SEED + 52, 256, 3)) * diag).astype(np.float32)
    q = np.concatenate([B._rotated(c, B.rotations(B.SEED + 53, 256), half), B.plank_records(lo, hi, 16, B.SEED + 54)])
    box = scene.grid_box(tris)
    want = {k: B.host_brute(exe, d, tris, q, k, grid=box) for k in (1, 8)}
    assert (want[8][1] == 9).sum() >= 32 and (want[8][1] == 0).sum() >= 16
    st = D.OracleStages(name, tris)
    for stage in D.stages_of(name):
        out = D.stage_grid(st, stage)
        arrays = _host.oracle_grid_arrays(st.grid)
        for k in (1, 8):
            for prune in (True, False):
                ids, counts, _ = B.host_walk(exe, d, arrays, tris, q, k, float_prune=prune)
                B.assert_answers_equal(ids, counts, *want[k], f"{name} {stage} k={k} float_prune={prune}")


def test_the_float_prune_on_thin_diagonal_planks(scenes, host):
    """the 128 planks (half extents 50 %, 2 %, 2 % of the diagonal, along the diagonals of the box) at k = 8: the same answers with the face-normal prune
    and with the integer range alone; with it no plank tests more triangles, and the family fewer than half -- a plank fills a few percent of its bounding
    box.  The per-query means are printed."""
    exe, d = host
    for name in B.SCENES:
        tris, q, _, _ = scenes[name]
        arrays = B.oracle_grid_arrays(B.oracle_grid(tris, False, False))
        planks = q[B.PLANK]
        ids, counts, on = B.host_walk(exe, d, arrays, tris, planks, B.KMAX)
        ids0, counts0, off = B.host_walk(exe, d, arrays, tris, planks, B.KMAX, float_prune=False)
        B.assert_answers_equal(ids, counts, ids0, counts0, f"{name}: planks with and without the float prune")
        print(f"{name}: per plank, with the prune {on[:, 1].mean():.1f} triangle tests and {on[:, 0].mean():.1f} cells; without {off[:, 1].mean():.1f} and {off[:, 0].mean():.1f}")
        assert (on[:, 1] <= off[:, 1]).all() and (on[:, 0] <= off[:, 0]).all()
        assert 2 * int(on[:, 1].sum()) < int(off[:, 1].sum()) and 2 * int(on[:, 0].sum()) < int(off[:, 0].sum())
        # at k = 8 a walk soon has its eight ids and tests little; the whole list (paged once more from the ninth id) shows the same
        far = planks.copy(); far["first"] = tris.shape[0] // 2
        _, _, on = B.host_walk(exe, d, arrays, tris, far, B.KMAX)
        _, _, off = B.host_walk(exe, d, arrays, tris, far, B.KMAX, float_prune=False)
        assert (on[:, 1] <= off[:, 1]).all() and 2 * int(on[:, 1].sum()) < int(off[:, 1].sum())
        # queries beyond 4 M: the float prune is switched off, the counts are those of the integer range
        _, _, a = B.host_walk(exe, d, arrays, tris, q[B.FAR], B.KMAX)
        _, _, b = B.host_walk(exe, d, arrays, tris, q[B.FAR], B.KMAX, float_prune=False)
        assert (a == b).all()


def test_rounding_on_scene_pairs(fixture, scenes, host):
    """on 1024 (query, triangle) pairs per scene whose bounding boxes meet: header and numpy agree pair by pair; how often the float decision says "meet"
    where the rational test says "apart", and the reverse, is printed.  Exactly touching pairs are those of the lattice test above, where
    "apart where exact says meet" is 0.  The scenes' records are rounded -- the oriented box of a mesh triangle has its neighbours' shared edges ON its side
    faces but for that rounding -- so no pair of theirs touches exactly and the grown bounding box cannot decide them: the counts are reported, not hidden.
    What is asserted: every disagreement, either way, is a contact within the query's own margin -- the exact test says "meet" for the box whose axes are
    eps longer and "apart" for the box whose axes are eps shorter (eps: the grid's margin, 2^-16 of its largest |coordinate|)."""
    exe, d = host
    for name in B.SCENES:
        tris, q, _, _ = scenes[name]
        pairs = fixture[name + "_pairs"]
        truth = np.unpackbits(fixture[name + "_pairs_truth"])[:B.NUM_SCENE_PAIRS].astype(bool)
        qa, tb = q[pairs[:, 0]], tris[pairs[:, 1]]
        assert (B.host_pairs(exe, d, qa, tb) == scene.obb_pairs(tb, qa)).all(), "header and numpy agree"
        got = B.pair_decision(tris, q, pairs)
        apart, meet = int((truth & ~got).sum()), int((got & ~truth).sum())
        print(f"{name}: {truth.sum()} of {truth.size} pairs meet exactly; apart where exact says meet: {apart}; meet where exact says apart: {meet}")
        assert truth.sum() > 100 and (~truth).sum() > 100
        differ = np.flatnonzero(got != truth)
        eps = float(np.abs(np.concatenate(scene.grid_box(tris))).max()) * 2.0 ** -16
        assert (B.exact_pairs(qa[differ], tb[differ]) == truth[differ]).all(), "the fixture's truth is the exact test's"
        assert B.exact_pairs(qa[differ], tb[differ], grow=eps).all() and not B.exact_pairs(qa[differ], tb[differ], grow=-eps).any(), "every disagreement is a contact within the margin"


def test_host_program_under_the_sanitizers(fixture, scenes, tmp_path):
    """the host program, built stand-alone with address and undefined-behaviour sanitizers, runs pairs, brute and walk clean"""
    exe = B.build_host(tmp_path, sanitize=True)
    tris, q, qlab, tlab = scenes["mesh"]
    obbs, ltris, _ = B.lattice_pairs()
    truth = np.unpackbits(fixture["lattice_truth"])[:B.NUM_LATTICE_PAIRS].astype(bool)
    assert (B.host_pairs(exe, tmp_path, obbs[:4096], ltris[:4096]) == truth[:4096]).all()
    arrays = B.oracle_grid_arrays(B.oracle_grid(tris, True, False))
    for k, any_ in ((B.KMAX, False), (1, True)):
        ids, counts, _ = B.host_walk(exe, tmp_path, arrays, tris, q, k, qlab, tlab, any_=any_)
        if not any_:
            B.assert_answers_equal(ids, counts, *B.expected(fixture, "mesh_lab", k), "the sanitized walk")
    sub = slice(B.FAR.start - 32, B.BAD.stop)
    ids, counts = B.host_brute(exe, tmp_path, tris, q[sub], 3)
    B.assert_answers_equal(ids, counts, B.expected(fixture, "mesh", 3)[0][sub], B.expected(fixture, "mesh", 3)[1][sub], "the sanitized brute force")


def test_kernel_resources_and_budget(fixture):
    """obb_tris_kernel as the compiler reports it: no scratch, no spill, 126 VGPRs (four wavefronts per SIMD); overlap_boxes_kernel beside it keeps its 128;
    at most 120 kernels in the library"""
    rows = _host.kernel_rows("overlap")
    assert rows["obb_tris_kernel"] == (126, 0, 0, 4), rows
    assert rows["overlap_boxes_kernel"] == (128, 0, 0, 4), rows
    text = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "overlap", "obb_tris"], capture_output=True, text=True, cwd=ROOT).stdout
    assert re.search(r"lds\s+8192\b", text), text
    c = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "count_kernels.py"), "-v"], capture_output=True, text=True, cwd=ROOT)
    m = re.search(r"(\d+) kernels in", c.stdout)
    assert m and int(m.group(1)) <= 120, c.stdout[-300:] + c.stderr[-300:]
    assert c.stdout.count("obb_tris_kernel") == 1 and c.stdout.count("overlap_boxes_kernel") == 1 and "max_ref_kernel" not in c.stdout
    src = open(os.path.join(ROOT, "hagrid_amd", "csrc", "overlap.hip")).read()
    entry = src[src.index('extern "C" int hagrid_overlap_obbs'):src.index('extern "C" int hagrid_overlap_boxes')]
    assert "obb_tris_kernel<<<" in entry and not re.search(r"pool_alloc<|\.get<|ctx_scan<", entry), "the entry point launches and makes no pool request"


def test_header_library_and_bindings(fixture):
    from hagrid_amd import api, lib
    text = open(os.path.join(ROOT, "include", "hagrid_amd.h")).read()
    assert re.search(r"int\s+hagrid_overlap_obbs\s*\(\s*hagrid_ctx\*\s*ctx,\s*const hagrid_grid\*\s*grid,\s*const void\*\s*tris,\s*const void\*\s*obbs,\s*int num_obbs,"
                     r"\s*const void\*\s*query_labels,\s*const void\*\s*tri_labels,\s*int k,\s*void\*\s*ids,\s*void\*\s*counts,\s*void\*\s*counters,\s*uint32_t flags\)", text)
    assert re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", text)
    assert "hagrid_overlap_obbs" in lib.SIGNATURES and len(lib.SIGNATURES["hagrid_overlap_obbs"][1]) == 12 and lib.ABI_VERSION == 3
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT hagrid_overlap_obbs\b", exported)
    for name in ("overlap_obbs", "obb_records", "tris_in_obbs"):
        assert name in api.__all__ and callable(getattr(api, name))
    assert callable(scene.overlap_obbs) and callable(scene.obb_pairs) and scene.OBB_DTYPE.itemsize == 64
    assert "overlap_obbs" in open(os.path.join(ROOT, "include", "hagrid", "traverse.h")).read()
    assert os.path.exists(os.path.join(ROOT, "include", "hagrid", "obb.h"))
