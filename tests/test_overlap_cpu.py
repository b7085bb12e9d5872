"""Box-overlap queries, the part that needs no GPU: the numpy statement hagrid_amd/scene.py against what the REFERENCE's own intersect_prim_cell returned
for recorded (triangle, box) pairs (AND the bounds check); the triangle / box test and the brute force of include/hagrid/overlap.h (compiled for the
host) against the fixture tests/golden/overlap.npz; the host walk tests/cpp/overlap_host.cpp -- the walk the gfx950 kernel runs -- over grids of the CPU
oracle against the fixture on every box, for k = 1, 2, 3, 5, 8, both cell formats and both expansion modes; the prefix property; paging; the lattice's
shared faces; the entry points in header, library and bindings."""
import os
import re
import subprocess

import numpy as np
import pytest

import _overlap as V
from hagrid_amd import scene

ROOT = V.ROOT
INC = V.INC


# The column sums of the walk's per-box counters (cells visited, tests evaluated, sub-blocks pruned) over the 4096 fixture boxes, by scene, for k = 8 and for
# k = 1 with ANY; both cell formats and both expansion modes give the same.  Taken at the parent of the commit that moved the descent into
# include/hagrid/block_walk.h: the order of the visits is part of a counter, so a walk that visits in another order misses these.
WALK_COUNTERS = {"soup": ((2194470, 88109, 1689033), (10876, 10294, 182760)), "mesh": ((494334, 91860, 2461577), (14319, 17235, 822295))}


def sums(totals):
    return tuple(int(v) for v in totals.sum(axis=0, dtype=np.int64))


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return np.load(V.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_host")
    return V.build_host(d), d


@pytest.fixture(scope="module")
def scenes(fixture):
    out = {}
    for name in V.SCENES:
        tris = V.make_tris(name)
        out[name] = (tris, V.scene_boxes(fixture, name, tris))
    return out


@pytest.fixture(scope="module")
def unbounded(fixture):
    """the boxes with infinite bounds of each scene, checked against the fixture's checksum"""
    out = {}
    for k, name in enumerate(V.SCENES):
        b = V.unbounded_boxes(V.make_tris(name), V.NUM_UNBOUNDED, V.BOX_SEED + 200 + k)
        assert V.box_sum(b) == int(fixture[name + "_unb_box_sum"])
        out[name] = b
    return out


def test_pairs_equal_the_reference_and_the_bounds_check(fixture, scenes, host):
    """scene.overlap_pairs and meets() of the header on the recorded pairs: the value the reference's intersect_prim_cell returned AND the bounds check"""
    exe, d = host
    for name in V.SCENES:
        tris, boxes = scenes[name]
        t = tris[fixture[name + "_pair_tri"]]; b = boxes[fixture[name + "_pair_box"]]
        ref = fixture[name + "_pair_ref"] != 0
        assert ref.size == V.NUM_PAIRS
        inside = V.bounds_check(t, b)
        want = ref & inside
        got = scene.overlap_pairs(t, b)
        assert (got == want).all(), f"{name}: {(got != want).sum()} pairs differ from the reference"
        assert (V.host_pairs(exe, d, t, b) == want).all(), f"{name}: the header differs from the reference"
        assert want.sum() > 400 and (~want).sum() > 400 and (ref & ~inside).sum() >= 10, "both answers occur, and the bounds check alone decides some pairs (rare: plane and nine cross axes find no separation, a box axis does)"


def test_fixture_is_the_statement_and_the_brute_force(fixture, scenes, unbounded, host):
    """the stored answers are what the header's brute force gives (every box, those with infinite bounds too; k = 1 and 8) and what scene.overlap_boxes gives
    (a slice of every section)"""
    exe, d = host
    for name in V.SCENES:
        tris, boxes = scenes[name]
        for k in (1, V.KMAX):
            ids, counts = V.host_brute(exe, d, tris, boxes, k)
            want_ids, want_counts = V.expected(fixture, name, k)
            V.assert_answers_equal(ids, counts, want_ids, want_counts, f"{name} k={k}: brute_force of overlap.h against the fixture")
            ids, counts = V.host_brute(exe, d, tris, unbounded[name], k)
            want_ids, want_counts = V.expected(fixture, name + "_unb", k)
            V.assert_answers_equal(ids, counts, want_ids, want_counts, f"{name} k={k}: brute_force of overlap.h against the fixture, infinite bounds")
        r = scene.overlap_boxes(tris, unbounded[name][:48], k=V.KMAX)
        assert (r["ids"] == fixture[name + "_unb_ids"][:48]).all() and (r["sizes"] == fixture[name + "_unb_sizes"][:48]).all()
        pick = np.concatenate([np.arange(s.start, s.stop)[:24] for s in (V.ONE, V.FINE, V.FIVE, V.TWENTY, V.LATTICE, V.POINT, V.PAGED)] + [np.arange(V.SPECIAL.start, V.SPECIAL.stop)])
        r = scene.overlap_boxes(tris, boxes[pick], k=V.KMAX)
        assert (r["ids"] == fixture[name + "_ids"][pick]).all() and (r["sizes"] == fixture[name + "_sizes"][pick]).all()
    assert os.path.getsize(V.FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "closest.npz"))


def test_fixture_semantics(fixture, scenes):
    for name in V.SCENES:
        tris, boxes = scenes[name]
        ids, sizes = fixture[name + "_ids"], fixture[name + "_sizes"]
        N = tris.shape[0]
        listed = ids >= 0
        assert (listed.sum(axis=1) == np.minimum(sizes, V.KMAX)).all(), "min(k, m) slots are used"
        assert (listed[:, :-1] >= listed[:, 1:]).all(), "the unused slots are the last ones"
        both = listed[:, :-1] & listed[:, 1:]
        assert (ids[:, 1:][both] > ids[:, :-1][both]).all(), "ascending, each id once"
        assert ids.max() < N
        # both sides of k and of k + 1, for every k tested
        for k in V.KS:
            assert (sizes < k).any() and (sizes == k).any() and (sizes == k + 1).any() and (sizes > k + 1).any(), (name, k)
        # every listed triangle meets its box
        bi, slot = np.nonzero(listed)
        clipped = scene.clip_boxes(boxes, *scene.grid_box(tris))
        assert scene.overlap_pairs(tris[ids[bi, slot]], clipped[bi]).all()
        inside = (boxes[:, 0:3] >= clipped[V.SPECIAL.start, 0:3]).all(axis=1) & (boxes[:, 4:7] <= clipped[V.SPECIAL.start, 4:7]).all(axis=1)
        assert inside.sum() > 2000 and (clipped[inside].view(np.uint32) == boxes[inside].view(np.uint32)).all(), "the clip leaves a box inside the grid alone"
        usz = fixture[name + "_unb_sizes"]
        assert usz.size == V.NUM_UNBOUNDED and (usz > V.KMAX + 1).sum() > 200 and (usz <= V.KMAX).sum() > 20
        sp = V.SPECIAL.start
        assert sizes[sp] == N or name == "soup", "the whole scene box meets every triangle of the mesh"
        assert sizes[sp] >= N - 8
        assert (sizes[sp + 1:sp + 7] > 0).any(), "boxes straddling a face of the grid meet triangles"
        assert (sizes[sp + 7:sp + 21] == 0).all(), "boxes beyond the grid meet nothing"
        assert (sizes[sp + 21:sp + 37] == 0).all() and (ids[sp + 21:sp + 37] == -1).all(), "inactive boxes"
        assert (sizes[sp + 53:sp + 56] == 0).all()
        assert (sizes[sp + 41:sp + 53] > 0).any(), "half-infinite boxes meet triangles"
        assert sizes[sp + 37] == sizes[sp], "the box infinite in every direction is the whole grid box"
        assert (sizes[V.POINT] > 0).sum() > 128, "points on the surface meet their triangle"
        # the paged boxes: ids above the third id of the box they repeat
        src = ids[V.PAGED_FROM:V.PAGED_FROM + 128]
        first = boxes[V.PAGED, 3].view(np.int32)
        assert (first == src[:, 2] + 1).all() and (first > 0).sum() > 64
        paged = ids[V.PAGED]
        assert (paged[paged >= 0] >= np.broadcast_to(first[:, None], paged.shape)[paged >= 0]).all()
        full = (src[:, 2] >= 0)
        assert (paged[full, :5] == src[full, 3:]).all(), "the page after the third id starts with the fourth"


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", V.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, scenes, unbounded, host, scene_name, compress, subset_only):
    """ids and counts equal for all 4096 boxes and the 384 with infinite bounds, for k = 1, 2, 3, 5, 8, over Cell and SmallCell grids of the CPU oracle,
    both expansion modes; the list for k is a prefix of the list for k + 1; the counters' sums for k = 8 and for ANY are the pinned ones"""
    exe, d = host
    tris, boxes = scenes[scene_name]
    G = V.oracle_grid(tris, compress, subset_only)
    assert (G.small_cells is not None) == compress
    arrays = V.oracle_grid_arrays(G)
    glo, ghi = scene.grid_box(tris)
    assert (arrays["bbox_min"].view(np.uint32) == glo.view(np.uint32)).all() and (arrays["bbox_max"].view(np.uint32) == ghi.view(np.uint32)).all(), "the fixture's grid box"
    inactive = ~((boxes[:, 0:3] <= boxes[:, 4:7]).all(axis=1))
    prev = None
    for k in V.KS:
        ids, counts, totals = V.host_walk(exe, d, arrays, tris, boxes, k)
        want_ids, want_counts = V.expected(fixture, scene_name, k)
        V.assert_answers_equal(ids, counts, want_ids, want_counts, f"{scene_name} compress={compress} subset_only={subset_only} k={k}")
        assert (totals[inactive] == 0).all() and inactive.sum() == 16
        if k == V.KMAX:
            assert sums(totals) == WALK_COUNTERS[scene_name][0]
        if prev is not None:
            assert (ids[:, :prev.shape[1]] == prev).all(), "the prefix property"
        prev = ids
        ids, counts, _ = V.host_walk(exe, d, arrays, tris, unbounded[scene_name], k)
        want_ids, want_counts = V.expected(fixture, scene_name + "_unb", k)
        V.assert_answers_equal(ids, counts, want_ids, want_counts, f"{scene_name} compress={compress} subset_only={subset_only} k={k}, infinite bounds")
    # ANY: some member of S exactly where S is not empty
    ids, counts, totals = V.host_walk(exe, d, arrays, tris, boxes, 1, any_=True)
    sizes = fixture[scene_name + "_sizes"]
    assert ((ids[:, 0] >= 0) == (sizes > 0)).all() and (counts == (sizes > 0)).all()
    assert sums(totals) == WALK_COUNTERS[scene_name][1]
    hit = ids[:, 0] >= 0
    assert scene.overlap_pairs(tris[ids[hit, 0]], scene.clip_boxes(boxes, glo, ghi)[hit]).all() and (ids[hit, 0] >= boxes[hit, 3].view(np.int32)).all()


@pytest.mark.parametrize("scene_name", V.SCENES)
def test_host_walk_equals_the_brute_force_for_unbounded_and_huge_boxes(scenes, host, scene_name):
    """1536 more boxes with one or two infinite bounds, and the same boxes with +-3e38, +-1e30 and +-1e6 in place of the infinities (bounds that would swallow
    the triangles' coordinates in the test if they were not clipped): the walk gives what the brute force gives, k = 8 and k = 2, and ANY finds a triangle
    exactly where there is one"""
    exe, d = host
    tris, _ = scenes[scene_name]
    unb = V.unbounded_boxes(tris, 1536, V.BOX_SEED + 300)
    arrays = V.oracle_grid_arrays(V.oracle_grid(tris, scene_name == "mesh", scene_name == "soup"))
    sets = [unb]
    for big in (3.0e38, 1.0e30, 1.0e6):
        b = unb.copy()
        c = b[:, (0, 1, 2, 4, 5, 6)]
        b[:, (0, 1, 2, 4, 5, 6)] = np.where(np.isinf(c), np.sign(c) * np.float32(big), c)
        sets.append(b)
    boxes = np.concatenate(sets)
    assert np.isinf(unb).any(axis=1).all() and np.isfinite(boxes[1536:]).all()
    for k in (V.KMAX, 2):
        w_ids, w_counts, _ = V.host_walk(exe, d, arrays, tris, boxes, k)
        b_ids, b_counts = V.host_brute(exe, d, tris, boxes, k)
        V.assert_answers_equal(w_ids, w_counts, b_ids, b_counts, f"{scene_name} k={k}: the walk against the brute force")
    n = unb.shape[0]
    assert (b_ids[:n] == b_ids[n:2 * n]).all() and (b_ids[:n] == b_ids[2 * n:3 * n]).all() and (b_ids[:n] == b_ids[3 * n:]).all(), "a bound beyond the grid is as good as an infinite one"
    a_ids, a_counts, _ = V.host_walk(exe, d, arrays, tris, boxes, 1, any_=True)
    assert ((a_ids[:, 0] >= 0) == (b_counts > 0)).all() and (a_counts == (b_counts > 0)).all()


def test_walk_is_no_brute_force(scenes, host):
    """over the 1 % boxes of the soup the walk evaluates fewer than N / 10 tests per box on average (a guard, not a target), and it prunes sub-blocks"""
    exe, d = host
    tris, boxes = scenes["soup"]
    G = V.oracle_grid(tris, False, True)
    _, _, totals = V.host_walk(exe, d, V.oracle_grid_arrays(G), tris, boxes, 8)
    print("per 1 % box: cells", totals[V.ONE, 0].mean(), "tests", totals[V.ONE, 1].mean(), "pruned", totals[V.ONE, 2].mean())
    assert totals[V.ONE, 1].mean() < tris.shape[0] / 10
    assert totals[V.ONE, 2].sum() > 0


def test_paging_reproduces_the_whole_list(scenes, host):
    """k = 3 and first = last id + 1, again and again, gives the brute-force list of 256 boxes (the first 128 of the 5 % and of the 1 % boxes), in order"""
    exe, d = host
    tris, boxes = scenes["soup"]
    pick = np.concatenate([np.arange(V.FIVE.start, V.FIVE.start + 128), np.arange(V.ONE.start, V.ONE.start + 128)])
    b = boxes[pick].copy()
    n = b.shape[0]
    arrays = V.oracle_grid_arrays(V.oracle_grid(tris, True, False))
    # the whole lists by the statement
    cb = scene.clip_boxes(b, *scene.grid_box(tris))
    full = [np.flatnonzero(scene.overlap_pairs(tris, np.broadcast_to(cb[i], (tris.shape[0], 8)))) for i in range(n)]
    assert max(len(f) for f in full) > 20
    pages = [[] for _ in range(n)]
    live = np.arange(n)
    for _ in range(64):
        ids, counts, _ = V.host_walk(exe, d, arrays, tris, b[live], 3)
        for row, i in enumerate(live):
            pages[i] += [int(v) for v in ids[row] if v >= 0]
        more = counts == 4
        assert (counts[~more] == (ids[~more] >= 0).sum(axis=1)).all()
        live = live[more]
        if live.size == 0:
            break
        b[live, 3] = (ids[more, 2] + 1).astype(np.int32).view(np.float32)
    assert live.size == 0
    for i in range(n):
        assert pages[i] == full[i].tolist(), f"box {pick[i]}"


def test_host_walk_under_sanitizers(fixture, scenes, tmp_path):
    """the host program with -fsanitize=address,undefined as a stand-alone binary: the walk (its stack is an array indexed at run time) over a SmallCell grid,
    the first 256 boxes of the soup, k = 8 and ANY"""
    exe = V.build_host(tmp_path, sanitize=True)
    tris, boxes = scenes["soup"]
    arrays = V.oracle_grid_arrays(V.oracle_grid(tris, True, True))
    ids, counts, _ = V.host_walk(exe, tmp_path, arrays, tris, boxes[:256], V.KMAX)
    want_ids, want_counts = V.expected(fixture, "soup", V.KMAX)
    V.assert_answers_equal(ids, counts, want_ids[:256], want_counts[:256], "sanitized walk")
    ids, counts, _ = V.host_walk(exe, tmp_path, arrays, tris, boxes[:256], 1, any_=True)
    assert ((ids[:, 0] >= 0) == (want_counts[:256] > 0)).all() and (counts == (want_counts[:256] > 0)).all()


def test_lattice_neighbours_share_their_faces():
    origin = np.float32([-1.3, 0.7, 11.1]); size = np.float32([0.1, 0.37, 1e-3]); n = (7, 5, 3)
    b = scene.lattice_boxes(origin, size, n)
    assert b.dtype == scene.BOX_QUERY_DTYPE and b.shape == (105,) and (b["first"] == 0).all() and (b["pad"] == 0).all()
    lo = b["min"].reshape(3, 5, 7, 3); hi = b["max"].reshape(3, 5, 7, 3)
    assert (lo[:, :, 1:, 0].view(np.uint32) == hi[:, :, :-1, 0].view(np.uint32)).all()
    assert (lo[:, 1:, :, 1].view(np.uint32) == hi[:, :-1, :, 1].view(np.uint32)).all()
    assert (lo[1:, :, :, 2].view(np.uint32) == hi[:-1, :, :, 2].view(np.uint32)).all()
    assert (lo[0, 0, 0] == origin).all() and (hi > lo).all()
    # x fastest, and the stated expression
    assert (b["min"][1] == np.float32([origin[0] + np.float32(1.0) * size[0], origin[1], origin[2]])).all()
    assert b["max"][104, 2] == origin[2] + np.float32(3.0) * size[2]


def test_records_and_entry_points(fixture):
    """the ctypes mirror: the record, the symbols declared in the header, exported by the library and bound"""
    from hagrid_amd import api, lib
    assert scene.BOX_QUERY_DTYPE.itemsize == 32
    assert [scene.BOX_QUERY_DTYPE.fields[k][1] for k in ("min", "first", "max", "pad")] == [0, 12, 16, 28]
    assert api.BOX_QUERY_DTYPE is scene.BOX_QUERY_DTYPE and api.OVERLAP_ANY == 1 == scene.OVERLAP_ANY and api.MAX_OVERLAP_IDS == 8
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "hagrid_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+hagrid_overlap_boxes\s*\(", code) and re.search(r"\bint\s+hagrid_overlap_lattice\s*\(", code)
    assert re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", code) and re.search(r"#define\s+HAGRID_OVERLAP_ANY\s+1u\b", code)
    L = lib.load()
    for name, nargs in (("hagrid_overlap_boxes", 10), ("hagrid_overlap_lattice", 11)):
        assert name in lib.SIGNATURES and hasattr(L, name) and len(lib.SIGNATURES[name][1]) == nargs
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code).group(1)
        assert len(decl.split(",")) == nargs, "the prototype has as many arguments as the header"
    for name in ("overlap_boxes", "voxelize", "BOX_QUERY_DTYPE"):
        assert hasattr(api, name) and name in api.__all__
    shim = open(os.path.join(INC, "hagrid", "traverse.h")).read()
    assert "overlap_boxes" in shim and "overlap_lattice" in shim
    prog = '#include "hagrid_amd.h"\nint main(void) { return (sizeof(&hagrid_overlap_boxes) && sizeof(&hagrid_overlap_lattice)) ? 0 : 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-fsyntax-only", "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_overlap_header_is_cxx11():
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC, "-fsyntax-only", "-x", "c++",
                        os.path.join(INC, "hagrid", "overlap.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
