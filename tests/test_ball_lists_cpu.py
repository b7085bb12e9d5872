"""Ball lists (hagrid_ball_refs, hagrid_unique_lists, hagrid_compact_lists), the part that needs no GPU: the numpy statements (scene.tris_within,
scene.unique_lists, scene.compact_lists), the headers under the host program tests/cpp/ball_lists_host.cpp and the fixture tests/golden/ball_lists.npz against
each other, bit for bit; the host walk with RefSink -- the walk the gfx950 kernel runs -- over grids of the CPU oracle, through the whole protocol, against the
brute force and against the concatenated pages of the k-list; labels on a mesh's own vertices; the deep grids of _deep_grids at every stage, once more under
sanitizers; the kernels' resources and the kernel budget; the entry points in header, library and bindings."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _ball_lists as BL
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
    return np.load(BL.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("ball_lists_host")
    return BL.build_host(d), d


@pytest.fixture(scope="module")
def san_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("ball_lists_san")
    return BL.build_host(d, sanitize=True), d


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name in K.SCENES:
        tris = K.make_tris(name)
        out[name] = (tris, BL.queries(tris))
    return out


_BRUTE = {}


def brute(scenes, host, name):
    """the host brute force over all 4096 queries of a scene: computed once, shared, never changed"""
    if name not in _BRUTE:
        exe, d = host
        tris, q = scenes[name]
        _BRUTE[name] = BL.host_brute(exe, d, tris, q)
        for v in _BRUTE[name].values():
            v.setflags(write=False)
    return _BRUTE[name]


# ---- stage 2 alone -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["plain", "san"])
def test_unique_and_compact_statement_header_and_host_agree(host, san_host, which):
    """the synthetic segments (lengths 0, 1, 2, 63, 64, 65, C - 1, C, C + 1, 3 C + 7, 20 000; heavy duplication, EMPTY, negative ids and NaN in the middle,
    +-0.0, refused ranges): the header's network for arbitrary n == scene.unique_lists, every word; compact into too little room likewise; nothing outside a
    segment changes.  Once more with the stand-alone sanitizer build."""
    exe, d = host if which == "plain" else san_host
    offsets, entries, capacity = BL.synthetic_segments()
    rooms = np.diff(offsets)
    for L in BL.SEGMENT_LENGTHS:
        assert (rooms == L).sum() >= 3 or L <= 2, L
    want_e, want_c = scene.unique_lists(offsets, entries)
    got_e, got_c = BL.host_unique(exe, d, offsets, entries)
    assert (got_c == want_c).all() and (BL.words(got_e) == BL.words(want_e)).all()
    # what the definition promises, on the statement's output
    first, room = scene._segment_ranges(offsets, capacity)
    owned = np.zeros(capacity, dtype=bool)
    for f, r, m in zip(first, room, want_c):
        seg = want_e[f:f + r]
        owned[f:f + r] = True
        assert (seg["id"][:m] >= 0).all() and np.unique(seg["id"][:m]).size == m and (BL.words(seg[m:]) == BL.words(scene.empty_entry())).all()
        assert ((seg["d2"][:m][:-1] < seg["d2"][:m][1:]) | ((seg["d2"][:m][:-1] == seg["d2"][:m][1:]) & (seg["id"][:m][:-1] < seg["id"][:m][1:]))).all()
    assert (~owned).sum() >= 5 and (BL.words(want_e)[~owned] == BL.POISON).all(), "slots of no segment are untouched"
    assert (want_c[room == 0] == 0).all() and (room == 0).sum() >= 7
    zero = want_e[want_e["d2"] == 0]
    assert np.signbit(zero["d2"]).any() and (~np.signbit(zero["d2"])).any(), "+0.0 and -0.0 both survive, bits unchanged"
    assert want_c.max() > BL.SORT_CAP and ((want_c > 64) & (want_c < BL.SORT_CAP)).any()
    out_offsets, out_capacity = BL.tight_destination(want_c)
    want_o = scene.compact_lists(offsets, want_e, want_c, out_offsets, out_capacity, fill=BL.poisoned(out_capacity))
    got_o = BL.host_compact(exe, d, offsets, got_e, got_c, out_offsets, BL.poisoned(out_capacity))
    assert (BL.words(got_o) == BL.words(want_o)).all()
    droom = scene._segment_ranges(out_offsets, out_capacity)[1]
    assert ((droom < want_c) & (droom > 0)).any() and (droom > want_c).any() and droom[-1] == 0 and want_c[-1] == 0


# ---- the definition ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.SCENES)
def test_statement_host_brute_force_and_fixture_agree(fixture, scenes, host, name):
    """ball_lists_host brute (RefSink under brute_force, then unique_segment) over all 4096 queries: the list lengths are the fixture's, the stored lists the
    fixture's bit for bit; scene.tris_within over the stored queries is the fixture's too -- which pins the brute force, the reference of the other tests, to the
    statement"""
    tris, q = scenes[name]
    assert int(fixture[name + "_query_sum"]) == int(K.bits(q).astype(np.uint64).sum()), "the fixture's queries are the generators' queries"
    b = brute(scenes, host, name)
    sizes = np.diff(b["offsets"])
    assert (sizes == fixture[name + "_sizes"]).all()
    want = BL.fixture_csr(fixture, name)
    BL.assert_csr_equal(BL.csr_slice(b, BL.STORED), want, f"{name}: brute force of closest.h against the fixture")
    BL.assert_csr_equal(scene.tris_within(tris, q[BL.STORED]), want, f"{name}: scene.tris_within against the fixture")
    trivial = (q[:, 3] < 0) | np.isnan(q).any(axis=1)
    assert trivial.sum() == 16 and (sizes[trivial] == 0).all()
    print(name, "listed", int(sizes.sum()), "median", int(np.median(sizes)), "longest", int(sizes.max()), "empty", int((sizes == 0).sum()))
    assert sizes.max() > 3 * BL.SORT_CAP and np.median(sizes) > 32 and (sizes == 0).sum() > 100
    assert os.path.getsize(BL.FIXTURE) < 400000


# ---- the walk --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", K.SCENES)
def test_host_walk_through_the_protocol(scenes, host, scene_name, compress, subset_only):
    """count, scan, fill, unique, scan, compact on the host over Cell and SmallCell grids of the CPU oracle, both expansion modes: the lists are the brute
    force's, bit for bit, for all 4096 queries; R_i >= m_i; the ids among a query's references are exactly its list's; equal ids carry equal d2 bits"""
    exe, d = host
    tris, q = scenes[scene_name]
    arrays = K.oracle_grid_arrays(K.oracle_grid(tris, compress, subset_only))
    got = BL.host_lists(exe, d, arrays, tris, q)
    want = brute(scenes, host, scene_name)
    BL.assert_csr_equal(got, want, f"{scene_name} compress={compress} subset_only={subset_only}")
    m = np.diff(want["offsets"])
    assert (got["refs"] >= m).all() and (got["refs"] > m).any()
    trivial = (q[:, 3] < 0) | np.isnan(q).any(axis=1)
    assert (got["counts"][trivial] == 0).all() and (got["counts"][~trivial, 1] >= 1).all()
    assert got["totals"][4] == got["refs"].sum() and got["totals"][5] == 0 and got["totals"][0] == q.shape[0]
    ro, re_ = got["ref_offsets"], got["ref_entries"]
    for i in list(range(K.RADIUS.start, K.RADIUS.start + 64)) + [K.UNIFORM.start, K.SPECIAL.start + 33]:
        r = re_[ro[i]:ro[i + 1]]
        ids, firsts = np.unique(r["id"], return_index=True)
        assert (ids == np.sort(want["ids"][want["offsets"][i]:want["offsets"][i + 1]])).all()
        assert (K.bits(r["d2"]) == K.bits(r["d2"][firsts][np.searchsorted(ids, r["id"])])).all()
    print(scene_name, "duplicate factor", got["refs"].sum() / max(1, m.sum()), "longest run of references", int(got["refs"].max()))


@pytest.mark.parametrize("scene_name", K.SCENES)
def test_lists_are_the_concatenated_pages(scenes, host, scene_name, tmp_path_factory):
    """the PAGED queries of _nearest_k (their radii are finite there already): the k-list of nearest_k_host paged to its end at k = 3 concatenates to the
    ball list; 30 and more queries take four pages and more (what test_nearest_k_cpu.MUST_PAGE pins for the same queries)"""
    exe, d = host
    nk = NK.build_host(tmp_path_factory.mktemp("ball_lists_nk"))
    tris, q = scenes[scene_name]
    arrays = K.oracle_grid_arrays(K.oracle_grid(tris, True, True))
    qs = q[NK.PAGED]
    got = BL.host_lists(exe, d, arrays, tris, qs)
    lists, pages = NK.page_through(lambda which, cursors: NK.host_walk(nk, d, arrays, tris, qs[which], NK.PAGE_K, cursors=cursors)[0], qs.shape[0], NK.PAGE_K)
    NK.assert_pages_equal_csr(lists, got, scene_name)
    assert (pages >= 4).sum() >= 30


def test_labels_on_the_meshs_own_vertices(host):
    """_nearest_k.stadium_labels: the walk through the protocol is scene.tris_within with the labels; no list holds a triangle the vertex belongs to; labels
    of -1 skip nothing"""
    exe, d = host
    tris, F, q, labels = NK.stadium_labels()
    arrays = K.oracle_grid_arrays(K.oracle_grid(tris, True, True))
    got = BL.host_lists(exe, d, arrays, tris, q, query_labels=labels, tri_labels=F)
    BL.assert_csr_equal(got, scene.tris_within(tris, q, query_labels=labels, tri_labels=F), "labelled walk against the statement")
    BL.assert_csr_equal(BL.host_brute(exe, d, tris, q, query_labels=labels, tri_labels=F), got, "labelled brute force against the walk")
    owner = np.repeat(np.arange(q.shape[0]), np.diff(got["offsets"]))
    assert not (F[got["ids"]] == labels[owner][:, None]).any(), "a list holds a triangle the vertex belongs to"
    plain = BL.host_lists(exe, d, arrays, tris, q)
    minus = BL.host_lists(exe, d, arrays, tris, q, query_labels=np.full(q.shape[0], -1, np.int32), tri_labels=F)
    BL.assert_csr_equal(minus, plain, "labels of -1 skip nothing")
    assert plain["ids"].size > got["ids"].size > 0


def deep_points(tris):
    """_deep_grids.points with every r = inf replaced by 20 % of the diagonal"""
    pts = D.points(tris)
    lo, hi = scene.tris_bbox(tris)
    pts[np.isposinf(pts[:, 3]), 3] = np.float32(0.2) * scene.bbox_diagonal(lo, hi)
    return pts


@pytest.mark.parametrize("name", D.WALKED)
def test_deep_grids_at_every_stage(host, san_host, name):
    """every scene and stage of _deep_grids.CATALOGUE: the protocol on the host against the host brute force, bit for bit; once more with the stand-alone
    sanitizer build of the host program (walk, network, compact)"""
    exe, d = host
    tris = D.make_tris(name)
    pts = deep_points(tris)
    want = BL.host_brute(exe, d, tris, pts)
    sizes = np.diff(want["offsets"])
    assert (sizes >= 2).sum() > D.NUM_POINTS // 4 and (sizes == 0).any()
    st = D.OracleStages(name, tris)
    for stage in D.stages_of(name):
        out = D.stage_grid(st, stage)
        G = out[0] if stage == "compress" else out
        arrays = _host.oracle_grid_arrays(G)
        for which, (e, dd) in (("plain", host), ("san", san_host)):
            BL.assert_csr_equal(BL.host_lists(e, dd, arrays, tris, pts), want, f"{name} after {stage} ({which})")


# ---- the library -------------------------------------------------------------------------------------------------------------------------

def test_kernel_resources_and_budget(fixture):
    """tools/kernel_resources.py: no scratch and no spill for the two new kernels, VGPRs and wavefronts per SIMD as found; the pinned rows of closest, capsule
    and overlap as they were; tools/count_kernels.py: at most 120 kernels, each new kernel once"""
    rows = _host.kernel_rows("ball_lists")
    assert set(rows) == {"ball_refs_kernel", "unique_lists_kernel"}, rows
    assert rows["ball_refs_kernel"] == (90, 0, 0, 5), rows
    assert rows["unique_lists_kernel"] == (66, 0, 0, 4), rows
    rows = _host.kernel_rows("closest")
    assert rows["closest_points_kernel"] == (94, 0, 0, 5) and rows["nearest_tris_kernel"] == (103, 0, 0, 4), rows
    rows = _host.kernel_rows("overlap")
    assert rows["obb_tris_kernel"] == (126, 0, 0, 4) and rows["overlap_boxes_kernel"] == (128, 0, 0, 4), rows
    capsule = _host.kernel_rows("capsule")
    assert set(capsule) == {"segment_tris_kernel"} and capsule["segment_tris_kernel"][1:3] == (0, 0), capsule
    c = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "count_kernels.py"), "-v"], capture_output=True, text=True, cwd=ROOT)
    m = re.search(r"(\d+) kernels", c.stdout)
    assert m and int(m.group(1)) <= 120, c.stdout[-300:] + c.stderr[-300:]
    for kernel in ("ball_refs_kernel", "unique_lists_kernel"):
        assert c.stdout.count(kernel) == 1, kernel


def test_entry_points_and_no_allocation_site(fixture):
    """the three symbols declared in the header, exported by the library and bound; ABI 3; the Python layer; ball_lists.hip asks for no memory"""
    from hagrid_amd import api, lib
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "hagrid_amd.h")).read(), flags=re.S)
    assert re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", code)
    L = lib.load()
    assert L.hagrid_abi_version() == lib.ABI_VERSION == 3
    for name, nargs in (("hagrid_ball_refs", 13), ("hagrid_unique_lists", 8), ("hagrid_compact_lists", 11)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in lib.SIGNATURES and hasattr(L, name) and len(lib.SIGNATURES[name][1]) == nargs, name
    for name in ("ball_refs", "unique_lists", "compact_lists", "ball_lists"):
        assert hasattr(api, name) and name in api.__all__
    for name in ("unique_lists", "compact_lists", "tris_within"):
        assert hasattr(scene, name)
    prog = '#include "hagrid_amd.h"\nint main(void) { return sizeof(&hagrid_ball_refs) + sizeof(&hagrid_unique_lists) + sizeof(&hagrid_compact_lists) ? 0 : 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-fsyntax-only", "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    source = open(os.path.join(ROOT, "hagrid_amd", "csrc", "ball_lists.hip")).read()
    for site in ("pool_alloc<", "pool_try_alloc<", ".get<", "ctx_scan<", "scan_plain(", "hagrid_mem_alloc(", "device_request(", "lookback_state(", "hipMalloc"):
        assert site not in source, site
    assert f"kSortCap = {BL.SORT_CAP};" in source
