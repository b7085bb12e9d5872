"""Deep and unfinished grids on the CPU (tests/_deep_grids.py): the catalogue's scenes have the depth they are listed with, before and after flatten; the
host statement of every query (tests/cpp) walked over the oracle's grid after build, merge, flatten, expand and compress equals its brute-force mode bit for
bit, and the oracle's traversal equals its brute force; the queries reach the paths they are meant to (paging, k + 1, empty answers); the host programs run
under the sanitizers on the grid of virtual resolution 65536 straight after build; a grid of 16 levels is built by every pass and refused by every walk."""
import subprocess

import numpy as np
import pytest

from hagrid_amd import scene

import _closest as K
import _crossing_lists as CL
import _crossings as X
import _deep_grids as D
import _host
import _multi_hit as M
import _overlap as V
import _overlap_tris as T


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    return D.build_hosts(tmp_path_factory.mktemp("deep_grids_hosts"))


@pytest.fixture(params=D.WALKED)
def deep(request, hosts):
    return D.brute_answers(hosts, request.param)


def assert_depth(G, name, stage):
    shift = D.CATALOGUE[name]["shift"]
    assert G.shift == shift, f"{name} {stage}: shift {G.shift}, the catalogue says {shift}"
    chain = D.longest_chain(G.entries, G.dims)
    if stage in ("build", "merge"):
        assert chain == shift, f"{name} {stage}: the longest chain of inner words is {chain}"
    else:
        assert 1 <= chain <= -(-shift // 3), f"{name} {stage}: the longest chain of inner words is {chain} after flatten"


def test_coverage_conditions(deep):
    """what keeps the comparisons below from passing on empty answers"""
    s = deep
    n = D.NUM_RAYS
    counts = s.records["id"]
    # (paging: a ray along a stack crosses its twelve plates.  `nested` has no stacks, and its rays keep away from the two inner clusters, where many
    # triangles lie on every line but the reference's test decides nothing (D.make_rays): there a few rays page, and most cross several triangles)
    if s.name == "nested":
        assert (counts > 8).any() and (counts > 1).sum() >= n // 2
    else:
        assert (counts > 8).sum() >= n // 2, f"{s.name}: {(counts > 8).sum()} of {n} rays have more than 8 crossings"
    assert (s.hits["id"] >= 0).sum() >= n // 2
    cnt = s.overlap[8][1]
    assert (cnt == 9).sum() >= D.NUM_BOXES // 4 and (cnt == 0).sum() >= D.NUM_BOXES // 10, f"{s.name}: {(cnt == 9).sum()} boxes at k + 1, {(cnt == 0).sum()} empty"
    assert (s.closest["id"] >= 0).sum() >= D.NUM_POINTS // 2 and (s.closest["id"] < 0).any()
    half = min(D.NUM_CONTACTS, s.tris.shape[0])
    assert s.contacts.shape[0] == 2 * half
    # (the lifted half of the contact queries cuts through the plates above it; the other half lies between two plates.  `nested` is a soup: no such promise)
    if s.name != "nested":
        assert (s.contact[1][half:] > 0).sum() >= half // 2 and (s.contact[1][:half] == 0).sum() >= half // 2
    assert (s.contact[1] > 0).any() and (s.contact[1] == 0).any()
    print(s.name, "rays with more than 8 crossings", int((counts > 8).sum()), "boxes at k + 1", int((cnt == 9).sum()), "empty boxes", int((cnt == 0).sum()),
          "points that find a triangle", int((s.closest["id"] >= 0).sum()), "contacts", int((s.contact[1] > 0).sum()))


def test_host_walks_equal_brute_force_at_every_stage(deep, hosts):
    """every stage the oracle accepts: the depth, then each host walk over the oracle's arrays against its brute-force mode, and the oracle's traversal
    against its brute force -- bit for bit.  The ray walks: bit for bit on s10 and s12.  On s15 and `nested` the reference's ray / triangle test accepts
    crossings that pass outside a tiny triangle (D.slack_crossings: its -1e-9 is a sixth of an s15 plate and more than a whole triangle of the innermost
    cluster), in voxels whose cells do not list it; a ray may differ from the brute force only if it has such a crossing, the nearest hit on under 1 % of
    the rays, any walk on no more rays than D.LEFT_OUT lists (measured there), and no more rays than it lists may carry such a crossing (D.compared)."""
    s = deep
    d = hosts["dir"]
    st = D.OracleStages(s.name, s.tris)
    for stage in D.STAGES:
        out = D.stage_grid(st, stage)
        if stage == "compress":
            assert out[1] == D.CATALOGUE[s.name]["compress"], f"{s.name}: compress"
            if not out[1]:
                assert st.grid.small_cells is None and st.grid.cells is not None
                continue
            assert st.grid.small_cells is not None
        G = st.grid
        what = f"{s.name} {stage}"
        assert_depth(G, s.name, stage)
        arrays = _host.oracle_grid_arrays(G)
        assert (G.bbox_min.view(np.uint32) == s.grid_box[0].view(np.uint32)).all() and (G.bbox_max.view(np.uint32) == s.grid_box[1].view(np.uint32)).all()
        # region queries
        got, _ = K.host_walk(hosts["closest"], d, arrays, s.tris, s.points)
        K.assert_results_equal(got, s.closest, what + ": closest points")
        for k in (1, 8):
            ids, cnt, _ = V.host_walk(hosts["overlap"], d, arrays, s.tris, s.boxes, k)
            V.assert_answers_equal(ids, cnt, *s.overlap[k], what + f": box overlap k={k}")
        ids, cnt, _ = V.host_walk(hosts["overlap"], d, arrays, s.tris, s.boxes, 1, any_=True)
        member = s.overlap[8][1] > 0
        assert ((ids[:, 0] >= 0) == member).all() and (cnt == member).all(), what + ": ANY"
        assert scene.overlap_pairs(s.tris[ids[member, 0]], scene.clip_boxes(s.boxes, *s.grid_box)[member]).all(), what + ": ANY returned a triangle outside its box"
        ids, cnt, _ = T.host_walk(hosts["contact"], d, arrays, s.tris, s.contacts, 8)
        T.assert_answers_equal(ids, cnt, *s.contact, what + ": contact queries")
        # ray queries
        hits, _ = G.traverse(s.tris, s.rays)
        nearest = (hits["id"] != s.hits["id"]) | (_host.bits(hits["t"]) != _host.bits(s.hits["t"]))
        differ = nearest.copy()
        rec = X.host_query(hosts["crossings"], d, s.tris, grid=arrays, page=8, rays=s.rays)["records"][:, 0]
        differ |= (X.rec_bits(rec) != X.rec_bits(s.records)).any(axis=1)
        lists = CL.host_lists(hosts["lists"], d, s.tris, s.rays, int(s.offsets[-1]), offsets=s.offsets, grid=arrays, page=8)
        assert (lists["guard"] == CL.POISON).all()
        differ |= CL.rays_that_differ(lists, s.lists, s.offsets)
        multi = M.host_walk(hosts["multi"], d, arrays, s.tris, s.rays, 8)
        differ |= (multi["id"] != s.multi[0]).any(axis=1) | (M.bits(multi["t"]) != M.bits(s.multi[1])).any(axis=1)
        print(what, "rays on which the traversal and the brute force differ:", int(nearest.sum()), "of", differ.size, "; on which any walk and its brute force differ:",
              int(differ.sum()), "; rays with a crossing by the slack:", int(s.slack.sum()))
        D.compared(s.name, nearest, s.slack, what + ": nearest hit", nearest=True)
        sure = D.compared(s.name, differ, s.slack, what + ": ray walks")
        # the walks against each other on the rays they are held to the brute force on: the nearest hit is the first of the k, the record counts what the
        # list holds.  (Not where the slack decides: the lists take a triangle from any cell that names it, the nearest-hit walk has stopped before.)
        assert (multi["id"][:, 0] == hits["id"])[sure].all() and (M.bits(multi["t"][:, 0]) == M.bits(hits["t"]))[sure].all(), what + ": multi-hit against the traversal"
        assert (np.minimum(rec["id"], 8) == (multi["id"] >= 0).sum(axis=1))[sure].all(), what + ": crossing count against the multi-hit list"
        has = (rec["id"] > 0) & sure
        assert (_host.bits(rec["t"][has]) == _host.bits(hits["t"][has])).all() and (hits["id"][~has & sure] < 0).all(), what + ": the first crossing against the traversal"
        # inside votes: the rays of the three default directions, then the votes of the points whose three rays are held to the brute force
        votes = X.host_query(hosts["crossings"], d, s.tris, grid=arrays, page=8, points=s.points)
        pdiff = (X.rec_bits(votes["records"]) != X.rec_bits(s.inside["records"])).any(axis=1)
        print(what, "point rays on which the walk and the brute force differ:", int(pdiff.sum()), "of", pdiff.size, "; with a crossing by the slack:", int(s.point_slack.sum()))
        psure = D.compared(s.name, pdiff, s.point_slack, what + ": inside votes", points=True).reshape(-1, 3).all(axis=1)
        assert (votes["inside"] == s.inside["inside"])[psure].all(), what + ": inside votes"


def test_host_programs_under_sanitizers_at_the_resolution_limit(hosts, tmp_path):
    """the stand-alone sanitized programs over the s15 grid straight after build: 15 look-up words per cell, voxel coordinates up to 65535"""
    s = D.brute_answers(hosts, "s15")
    st = D.OracleStages("s15", s.tris)
    arrays = _host.oracle_grid_arrays(D.stage_grid(st, "build"))
    d = tmp_path
    san = D.build_hosts(d, sanitize=True)
    got, _ = K.host_walk(san["closest"], d, arrays, s.tris, s.points)
    K.assert_results_equal(got, s.closest, "sanitized closest points")
    ids, cnt, _ = V.host_walk(san["overlap"], d, arrays, s.tris, s.boxes, 8)
    V.assert_answers_equal(ids, cnt, *s.overlap[8], "sanitized box overlap")
    ids, cnt, _ = T.host_walk(san["contact"], d, arrays, s.tris, s.contacts, 8)
    T.assert_answers_equal(ids, cnt, *s.contact, "sanitized contact queries")
    sure = ~s.slack            # (the bounded set is asserted above, stage by stage; here the programs run for the sanitizers)
    rec = X.host_query(san["crossings"], d, s.tris, grid=arrays, page=8, rays=s.rays)["records"][:, 0]
    X.assert_records_equal(rec[sure], s.records[sure], "sanitized crossings")
    lists = CL.host_lists(san["lists"], d, s.tris, s.rays, int(s.offsets[-1]), offsets=s.offsets, grid=arrays, page=8)
    assert not (CL.rays_that_differ(lists, s.lists, s.offsets) & sure).any() and (lists["guard"] == CL.POISON).all()
    multi = M.host_walk(san["multi"], d, arrays, s.tris, s.rays, 8)
    assert (multi["id"] == s.multi[0])[sure].all() and (M.bits(multi["t"]) == M.bits(s.multi[1]))[sure].all()


def test_sixteen_levels_are_built_and_refused_by_every_walk(hosts, capfd):
    """s16: the oracle builds, merges, flattens and expands it, compress says no, and every host walk refuses its header"""
    tris = D.make_tris("s16")
    st = D.OracleStages("s16", tris)
    for stage in D.STAGES[:-1]:
        G = D.stage_grid(st, stage)
        assert_depth(G, "s16", stage)
        assert G.num_cells > 0 and G.cells is not None
    G, ok = D.stage_grid(st, "compress")
    assert ok is False and G.small_cells is None and G.cells is not None and G.shift == 16
    arrays = _host.oracle_grid_arrays(G)
    d = hosts["dir"]
    rays, boxes, points, contacts = D.make_rays("s16", tris, 64), D.make_boxes("s16", tris), D.points(tris), D.contact_queries("s16", tris)
    calls = {"closest": lambda: K.host_walk(hosts["closest"], d, arrays, tris, points),
             "overlap": lambda: V.host_walk(hosts["overlap"], d, arrays, tris, boxes, 8),
             "contact": lambda: T.host_walk(hosts["contact"], d, arrays, tris, contacts, 8),
             "crossings": lambda: X.host_query(hosts["crossings"], d, tris, grid=arrays, page=8, rays=rays),
             "lists": lambda: CL.host_lists(hosts["lists"], d, tris, rays, 64, stride=1, grid=arrays, page=8),
             "multi": lambda: M.host_walk(hosts["multi"], d, arrays, tris, rays, 8)}
    for name, call in calls.items():
        capfd.readouterr()
        with pytest.raises(subprocess.CalledProcessError) as e:
            call()
        assert e.value.returncode == 2, name
        assert "bad shift" in capfd.readouterr().err, name
