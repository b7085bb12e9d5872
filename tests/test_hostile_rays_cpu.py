"""The CPU oracle's walk on the hostile-ray catalogue (tests/_hostile_rays.py): termination below the step cap, the contract of DESIGN.md section 2 for
inadmissible rays, zero signs, and the walk against the reference brute force -- bit for bit on the soup (tier 1), through the float64 evaluation
where the two differ on the mesh (tier 2).  The kernels are pinned to this oracle by tests/test_hostile_rays_gpu.py."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

import _crossings as X
import _hostile_rays as H
import _multi_hit as M

CASES = [(name, grid, compress) for name in H.SCENES for grid in H.GRID_PARAMS for compress in (False, True)]
IDS = [f"{n}-{g}-{'small' if c else 'cell'}" for n, g, c in CASES]


def words(hits) -> np.ndarray:
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def _tris(name):
    return H.make_tris(name)


@functools.lru_cache(maxsize=None)
def _case(name, grid, compress):
    tris = _tris(name)
    G = H.oracle_grid(tris, H.GRID_PARAMS[grid], compress)
    rays, fam = H.catalogue(tris, G)
    return tris, G, rays, fam


@functools.lru_cache(maxsize=None)
def _brute(name, grid):
    """the reference brute force of a catalogue: computed through the reference-header harness where it was built (and then equal to the fixture),
    the fixture otherwise"""
    tris, G, rays, fam = _case(name, grid, False)
    fx = H.fixture_hits(np.load(H.FIXTURE), name, grid, rays)
    if O.ref_lib() is not None:
        bf = O.brute_force(tris, rays, nthreads=8, use_ref=True)
        assert (words(bf)[:, 0:2] == words(fx)[:, 0:2]).all(), "the fixture is the reference brute force"
    return fx


def _equal(a, b):
    return (a["id"] == b["id"]) & (H.bits(a["t"]) == H.bits(b["t"]))


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_every_catalogue_ray_terminates_in_both_conversion_modes(name, grid, compress):
    """No ray reaches the oracle's step cap, whether the walk converts float to int as x86 does or as the device does, through the single-threaded
    entry, the threaded one and the any-hit / barycentric variant; and the two conversion modes give the same records and step counts."""
    tris, G, rays, fam = _case(name, grid, compress)
    O.walk_capped()
    got = {}
    for mode in (0, O.DEVICE_F2I):
        with O.walk_mode(mode):
            hits, stats, steps = G.traverse(tris, rays, want_steps=True)
            threaded, _ = G.traverse(tris, rays, nthreads=4)
            ex = G.traverse_ex(tris, rays, O.ANY_HIT | O.UVS, nthreads=4)
        assert O.walk_capped() == (0, -1), (name, grid, compress, mode)
        assert (words(hits) == words(threaded)).all()
        got[mode] = (hits, stats, steps, ex)
    a, b = got[0], got[O.DEVICE_F2I]
    assert (words(a[0]) == words(b[0])).all() and a[1] == b[1] and (a[2] == b[2]).all() and (words(a[3]) == words(b[3])).all()
    res = np.array(G.dims) << G.shift
    assert a[1]["cells"] > 0 and a[2].max() > 1 and int(res.sum()) + 1 > 3


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_inadmissible_rays_are_misses_with_zero_steps(name, grid, compress):
    """family (j): id -1, t = the bits of the ray's tmax, u = v = 0, step count 0, not counted in rays_hit_grid -- also as a batch of their own and with the
    variant flags -- and what the other rays of the batch get does not depend on them"""
    tris, G, rays, fam = _case(name, grid, compress)
    j = fam == "j"
    assert j.sum() > 300
    want = H.contract_records(rays[j])
    for mode in (0, O.DEVICE_F2I):
        with O.walk_mode(mode):
            hits, stats, steps = G.traverse(tris, rays, want_steps=True)
            alone, alone_stats, alone_steps = G.traverse(tris, rays[j], want_steps=True)
            ex = G.traverse_ex(tris, rays[j], O.ANY_HIT | O.UVS, nthreads=2)
            others, others_stats, others_steps = G.traverse(tris, rays[~j], want_steps=True)
        assert (words(hits[j]) == want).all() and (steps[j] == 0).all()
        assert (words(alone) == want).all() and (alone_steps == 0).all() and (words(ex) == want).all()
        assert alone_stats["rays"] == j.sum() and all(v == 0 for k, v in alone_stats.items() if k != "rays"), alone_stats
        assert (words(hits[~j]) == words(others)).all() and (steps[~j] == others_steps).all()
        assert stats["rays_hit_grid"] == others_stats["rays_hit_grid"] and stats["cells"] == others_stats["cells"]


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_the_sign_of_a_zero_component_changes_nothing(name, grid, compress):
    """family (b) (-0) gets the records of family (a) (+0) bit for bit, steps included, and both get the brute force's"""
    tris, G, rays, fam = _case(name, grid, compress)
    a, b = fam == "a", fam == "b"
    assert (rays[a][:, 4:7] == rays[b][:, 4:7]).all() and (np.signbit(rays[b][:, 4:7]) & (rays[b][:, 4:7] == 0)).any(axis=1).all()
    hits, _, steps = G.traverse(tris, rays, want_steps=True)
    assert (words(hits[a]) == words(hits[b])).all() and (steps[a] == steps[b]).all()
    bf = _brute(name, grid)
    assert _equal(hits[a], bf[a]).all() and _equal(hits[b], bf[b]).all() and (bf["id"][a] >= 0).sum() > 100
    ex = G.traverse_ex(tris, rays, O.UVS)
    assert (words(ex[a]) == words(ex[b])).all()


@pytest.mark.parametrize("grid", list(H.GRID_PARAMS))
@pytest.mark.parametrize("compress", [False, True])
def test_tier1_soup_walk_equals_the_reference_brute_force(grid, compress):
    """families a - h on the soup: id and t of the walk are the reference brute force's, bit for bit; every family holds rays that hit"""
    tris, G, rays, fam = _case("soup", grid, compress)
    hits, _ = G.traverse(tris, rays, nthreads=4)
    bf = _brute("soup", grid)
    assert (fam == "h").sum() == 16 * len(H.WINDOWS) + 6 * 64, "family (h) found its 64 rays that hit"
    for f in "abcdefgh":
        m = fam == f
        bad = m & ~_equal(hits, bf)
        assert not bad.any(), (f, int(bad.sum()), np.flatnonzero(bad)[:5], hits[bad][:3], bf[bad][:3])
        assert (bf["id"][m] >= 0).sum() >= 64 and (bf["id"][m] < 0).sum() >= 8, f


def test_tier2_tolerance_is_the_measured_one():
    """T_DEV_MEASURED: the brute force's t against the float64 t of the same triangle over the generic family, in both scenes"""
    for name in H.SCENES:
        tris = _tris(name)
        rays = H.generic_rays(tris)
        bf = O.brute_force(tris, rays, nthreads=8, use_ref=O.ref_lib() is not None)
        has = bf["id"] >= 0
        assert has.sum() > 4000
        t64, _, _ = H.hits_f64(tris, rays[has], bf["id"][has].astype(np.int64))
        dev = np.abs(bf["t"][has].astype(np.float64) - t64) / np.maximum(np.abs(t64), H.t_unit(tris, rays)[has])
        print(name, "largest deviation of the brute force's t from float64 on the generic family:", dev.max())
        assert dev.max() <= H.T_DEV_MEASURED and H.T_TOL == 4 * H.T_DEV_MEASURED
        j = H.judge_f64(tris, rays[:1024], bf[:1024])
        assert j["real"].all() and not j["ambiguous"].any() and not j["missed"].any(), "the generic family passes both conditions without exception"


@pytest.mark.parametrize("grid", list(H.GRID_PARAMS))
@pytest.mark.parametrize("compress", [False, True])
def test_tier2_mesh_walk_against_brute_force_and_float64(grid, compress):
    """The mesh: the walk equals the brute force except on rays through shared edges and vertices and along triangle planes.  Where the two differ the float64 evaluation decides: the walk's record is a real intersection of that triangle at that t
    (condition 1) and no clearly nearer surface was passed by (condition 2).  Rays whose reported triangle is coplanar to them are ambiguous and left
    out: at most AMBIGUOUS_CAP of family (k) -- for the walk and for the brute force alone -- and none of any other family."""
    tris, G, rays, fam = _case("mesh", grid, compress)
    hits, _ = G.traverse(tris, rays, nthreads=4)
    bf = _brute("mesh", grid)
    diff = ~_equal(hits, bf)
    for f in "abcdefgh":
        m = fam == f
        assert not (m & diff).any(), (f, np.flatnonzero(m & diff)[:5])          # in general position to the mesh: tier 1 holds here too
        assert (bf["id"][m] >= 0).sum() >= 64
    k = fam == "k"
    assert not (diff & ~k & ~np.isin(fam, ["i", "j", "l"])).any()          # (j: the contract's record, not the brute force's; l: no brute force to speak of)
    # the brute force alone on family (k): how much of it float64 cannot judge
    jb = H.judge_f64(tris, rays[k], bf[k])
    print("family (k):", int(k.sum()), "rays,", int((diff & k).sum()), "differ; ambiguous by the brute force's own record:", int(jb["ambiguous"].sum()))
    assert jb["ambiguous"].sum() <= H.AMBIGUOUS_CAP * k.sum()
    d = diff & k
    assert d.any(), "the family is aimed at what makes walk and brute force differ"
    jw = H.judge_f64(tris, rays[d], hits[d]); jd = H.judge_f64(tris, rays[d], bf[d])
    left_out = jw["ambiguous"] | jd["ambiguous"]
    tie = H.bits(hits["t"][d]) == H.bits(bf["t"][d])
    print("  of the differing rays:", int(left_out.sum()), "coplanar (left out),", int((tie & ~left_out).sum()), "equal t with another id,", int((~tie & ~left_out).sum()), "another t")
    assert left_out.sum() <= H.AMBIGUOUS_CAP * k.sum()
    assert jw["real"][~left_out].all(), ("condition 1", np.flatnonzero(d)[~left_out & ~jw["real"]][:5])
    assert not jw["missed"][~left_out].any(), ("condition 2", np.flatnonzero(d)[~left_out & jw["missed"]][:5])
    # ... and wherever the brute force's minimum is unique and not coplanar the two agree: a difference is a second triangle at the very same t (a tie: the
    # brute force keeps the lowest id of all, the walk the lowest of the cell it ends in) or at another t within the tolerance across a shared edge or vertex
    # (the brute force's own record is then not clearly inside its triangle)
    decided = np.flatnonzero(d)[~left_out]
    multiplicity = H.minimum_multiplicity(tris, rays[decided])
    print("  triangles float64 finds within the tolerance of the nearest, per differing ray:", np.bincount(multiplicity).tolist())
    assert (multiplicity >= 2).all(), ("a difference where the float64 minimum is unique", decided[multiplicity < 2][:5])
    rest = np.flatnonzero(d)[~left_out & ~tie]
    t64, (b0, b1, b2), _ = H.hits_f64(tris, rays[rest], bf["id"][rest].astype(np.int64))
    assert (np.minimum(b0, np.minimum(b1, b2)) < H.EDGE_MARGIN).all(), "a difference away from every edge"


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_far_origins_report_real_intersections(name, grid, compress):
    """family (i), origins 1e3 .. 1e6 box diagonals away: float32 cannot resolve t there, so the walk is held to float64 alone -- the reported point lies on the
    reported triangle to within FAR_TOL * distance / |cos|.  (The brute force is printed for comparison; the kernels equal the walk bit for bit.)"""
    tris, G, rays, fam = _case(name, grid, compress)
    m = fam == "i"
    hits, _ = G.traverse(tris, rays[m])
    off = H.judge_far(tris, rays[m], hits)
    print("family (i): the walk's worst point is", off.max(), "of the bound off its triangle; the brute force's", H.judge_far(tris, rays[m], _brute(name, grid)[m]).max())
    assert (hits["id"] >= 0).sum() > 128 and off.max() <= 1.0


@pytest.mark.parametrize("name", H.SCENES)
def test_the_reference_prologue_loses_hits_and_walks_without_end(name):
    """What the classification is for: with the reference's prologue (O.NO_ADMISSION) family (b) loses hits the brute force finds, and members of family (j)
    are ended by the oracle's step cap -- more of them with the device's conversions, which take away the escape through INT_MIN -- instead of ending
    themselves.  Every other family does not notice the classification."""
    tris, G, rays, fam = _case(name, "default", False)
    bf = _brute(name, "default")
    with_it, _ = G.traverse(tris, rays, nthreads=4)
    capped = {}
    O.walk_capped()
    for mode in (O.NO_ADMISSION, O.NO_ADMISSION | O.DEVICE_F2I):
        with O.walk_mode(mode):
            hits, _ = G.traverse(tris, rays, nthreads=4)
        capped[mode], first = O.walk_capped()
        assert capped[mode] > 0 and fam[first] == "j", (mode, capped[mode], first)
        b = fam == "b"
        assert ((bf["id"][b] >= 0) & (hits["id"][b] < 0)).sum() > 50
        same = ~np.isin(fam, ["b", "c", "d", "e", "f", "j", "k", "l"])          # (families with -0 components differ; so may -0 next to planes)
        assert (words(hits[same]) == words(with_it[same])).all()
    assert capped[O.NO_ADMISSION | O.DEVICE_F2I] > capped[O.NO_ADMISSION]


def test_batches_put_hostile_rays_where_wavefronts_differ():
    """embed(): one wavefront all hostile, one with a single hostile ray in lane 0, one with it in lane 63, a length that is no multiple of 64"""
    tris, G, rays, fam = _case("soup", "default", False)
    batch, pos = H.embed(rays, G.bbox_min, G.bbox_max)
    hostile = np.zeros(batch.shape[0], bool); hostile[pos] = True
    assert batch.shape[0] % 64 != 0 and hostile.sum() == rays.shape[0] and (H.bits(batch[pos]) == H.bits(rays)).all()
    assert hostile[0:64].all() and hostile[64] and not hostile[65:128].any() and hostile[191] and not hostile[128:191].any()
    assert H._admissible(batch[~hostile]).all()
    inadmissible = ~H._admissible(batch)
    per_wave = np.add.reduceat(inadmissible.astype(int), np.arange(0, batch.shape[0], 64))
    assert (per_wave > 0).sum() > 20 and (fam[np.argsort(pos)][:64] != fam[np.argsort(pos)][0]).any(), "families are mixed within wavefronts"


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_skew_rays_need_the_saturating_conversion(name, grid, compress):
    """H.skew_rays (not part of the catalogue): one component 1e-12 .. 1e-36 of the others, the origin one ulp off a voxel plane of that axis.  With the device's
    conversions the walk ends below the cap and equals the reference brute force bit for bit; with the C cast of x86 it ends too, and how many hits it loses
    is printed ("What remains")."""
    tris, G, _, _ = _case(name, grid, compress)
    rays = H.skew_rays(tris, G)
    assert H._admissible(rays).all()
    bf = O.brute_force(tris, rays, nthreads=8, use_ref=O.ref_lib() is not None)
    O.walk_capped()
    x86, _ = G.traverse(tris, rays, nthreads=4)
    with O.walk_mode(O.DEVICE_F2I):
        dev, _ = G.traverse(tris, rays, nthreads=4)
    assert O.walk_capped() == (0, -1)
    print("skew rays:", rays.shape[0], "of which", int((bf["id"] >= 0).sum()), "hit; the x86 cast differs from the brute force on", int((~_equal(x86, bf)).sum()))
    assert _equal(dev, bf).all() and (bf["id"] >= 0).sum() > 256


@pytest.fixture(scope="module")
def multi_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("multi_hit_host")
    return M.build_host(d), d


@functools.lru_cache(maxsize=None)
def _skew_lists(name, grid):
    """the 8 nearest intersections of every skew ray by the brute force of tests/_multi_hit.py (the rays depend on the grid's planes, not on the cell format)"""
    tris, G, _, _ = _case(name, grid, False)
    rays = H.skew_rays(tris, G)
    return (rays,) + M.lists_by_brute_force(tris, rays, k=8)


@pytest.mark.parametrize("name,grid,compress", CASES, ids=IDS)
def test_multi_hit_host_walk_on_skew_rays(name, grid, compress, multi_host):
    """The contract test_skew_rays_need_the_saturating_conversion holds the oracle's device-conversion mode to, for the multi-hit host walk: on H.skew_rays its
    records are the k nearest of the brute force, id and t bit for bit, k = 1 and 8, both cell formats.  The walk converts the exit voxel through f2i of
    include/hagrid/cell_walk.h; with the plain cast it had before, the conversion was undefined on these rays and up to 20 of the 768 differed."""
    tris, G, _, _ = _case(name, grid, compress)
    rays, ids, t = _skew_lists(name, grid)
    assert (H.bits(rays) == H.bits(H.skew_rays(tris, G))).all() and rays.shape[0] == 768 and (ids[:, 0] >= 0).sum() > 256
    exe, d = multi_host
    for k in (1, 8):
        got = M.host_walk(exe, d, M.oracle_grid_arrays(G), tris, rays, k)
        bad = (got["id"] != ids[:, :k]).any(axis=1) | (M.bits(got["t"]) != M.bits(t[:, :k])).any(axis=1)
        assert not bad.any(), f"k={k}: {bad.sum()} of {bad.size} rays differ, first at {np.flatnonzero(bad)[:5]}"


def test_host_walks_under_sanitizers(multi_host, tmp_path):
    """multi_hit_host and crossings_host as stand-alone binaries with -fsanitize=address,undefined,float-cast-overflow, once each over the skew rays and the
    catalogue (SmallCells, the default grid): no report, and the records of the plain builds bit for bit"""
    tris, G, cat, fam = _case("soup", "default", True)
    arrays = M.oracle_grid_arrays(G)
    rays = np.concatenate([H.skew_rays(tris, G), cat])
    plain, d = multi_host
    want = M.host_walk(plain, d, arrays, tris, rays, 8)
    got = M.host_walk(M.build_host(tmp_path, sanitize=True), tmp_path, arrays, tris, rays, 8)
    assert (words(got) == words(want)).all() and (got["id"][:768, 0] >= 0).sum() > 256
    want = X.host_query(X.build_host(tmp_path), tmp_path, tris, grid=arrays, page=3, rays=rays)
    got = X.host_query(X.build_host(tmp_path, sanitize=True), tmp_path, tris, grid=arrays, page=3, rays=rays)
    X.assert_records_equal(got["records"], want["records"], "sanitized crossings walk")
    assert (got["totals"] == want["totals"]).all() and got["excess"] <= 0
