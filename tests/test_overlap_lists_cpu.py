"""Overlap lists (hagrid_box_refs, hagrid_tri_refs, hagrid_obb_refs, then hagrid_unique_lists and hagrid_compact_lists), the part that needs no GPU: the numpy
statements (scene.box_lists, scene.contact_lists, scene.obb_lists), RefList of include/hagrid/overlap.h under the host program tests/cpp/overlap_lists_host.cpp
and the fixtures of the three k-list queries (tests/golden/{overlap,overlap_tris,obb}.npz: |S| and the first eight ids of all 4096 queries per scene) against
each other; the host walk -- the walk the gfx950 kernel runs -- through the whole protocol over grids of the CPU oracle against the brute force; labels; paged
queries; the deep grids of _deep_grids at every stage, once more under sanitizers; the kernels' resources and the kernel budget; the entry points in header,
library and bindings.  Nothing here takes a tolerance: ids and counts are integers and every comparison is equality."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _deep_grids as D
import _host
import _overlap_lists as OL
from hagrid_amd import scene

ROOT = OL.ROOT
INC = OL.INC


@pytest.fixture(scope="module")
def fixtures():
    import __graft_entry__ as g
    g.build()
    return {shape: np.load(path) for shape, path in OL.FIXTURES.items()}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_lists_host")
    return OL.build_host(d), d


@pytest.fixture(scope="module")
def san_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_lists_san")
    return OL.build_host(d, sanitize=True), d


@pytest.fixture(scope="module")
def scenes():
    return {name: OL.make_tris(name) for name in OL.SCENES}


_BRUTE, _GRIDS = {}, {}


def brute(fixtures, scenes, host, shape, name, labelled=False):
    """the host brute force over all 4096 queries of a shape and scene: computed once, shared, never changed"""
    key = (shape, name, labelled)
    if key not in _BRUTE:
        exe, d = host
        b = OL.fixture_batch(shape, fixtures[shape], name, scenes[name], labelled)
        _BRUTE[key] = OL.host_brute(exe, d, scenes[name], b)
        for v in _BRUTE[key].values():
            v.setflags(write=False)
    return _BRUTE[key]


def oracle_arrays(scenes, name, compress, subset_only):
    key = (name, compress, subset_only)
    if key not in _GRIDS:
        _GRIDS[key] = OL.oracle_grid_arrays(OL.oracle_grid(scenes[name], compress, subset_only))
    return _GRIDS[key]


# ---- the definition ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", OL.SCENES)
@pytest.mark.parametrize("shape", OL.SHAPES)
def test_statement_host_brute_force_and_fixture_agree(fixtures, scenes, host, shape, name):
    """per shape and scene: scene.*_lists == RefList under the brute force of overlap.h / obb.h, then unique_segment == the fixture of the k-list query (every
    list's length is its `sizes`, its first min(8, length) ids are its `ids`) -- which pins the brute force, the reference of the other tests"""
    tris = scenes[name]
    b = OL.fixture_batch(shape, fixtures[shape], name, tris)
    got = brute(fixtures, scenes, host, shape, name)
    OL.assert_fixture(got, fixtures[shape], name, f"{shape} {name}: the host brute force")
    st = b.statement(tris)
    OL.assert_csr_equal(st, got, f"{shape} {name}: the statement against the host brute force")
    sizes = np.diff(got["offsets"])
    assert (np.diff(got["ids"])[np.setdiff1d(np.arange(got["ids"].size - 1), got["offsets"][1:-1] - 1)] > 0).all(), "every list ascends, each id once"
    print(shape, name, "listed", int(sizes.sum()), "longest", int(sizes.max()), "longer than the sort capacity", int((sizes > OL.SORT_CAP).sum()), "empty", int((sizes == 0).sum()))
    if shape != "contact":
        assert (sizes > OL.SORT_CAP).sum() >= 8
    else:
        assert sizes.max() > 200


# ---- the walk --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("name", OL.SCENES)
@pytest.mark.parametrize("shape", OL.SHAPES)
def test_host_walk_through_the_protocol(fixtures, scenes, host, shape, name, compress, subset_only):
    """count, scan, fill, unique, scan, compact on the host over Cell and SmallCell grids of the CPU oracle, both expansion modes: the lists are the brute
    force's for all 4096 queries; R_i >= m_i, R_i > m_i for some query; the ids among a query's references are exactly its list's; totals[4] is the sum of R,
    totals[5] is 0; the global-memory sort, the LDS sort and the 0 / 1 path of the second stage are all reached"""
    exe, d = host
    tris = scenes[name]
    b = OL.fixture_batch(shape, fixtures[shape], name, tris)
    got = OL.host_lists(exe, d, oracle_arrays(scenes, name, compress, subset_only), tris, b)
    want = brute(fixtures, scenes, host, shape, name)
    OL.assert_csr_equal(got, want, f"{shape} {name} compress={compress} subset_only={subset_only}")
    m = np.diff(want["offsets"]); R = got["refs"]
    assert (R >= m).all() and (R > m).any()
    assert got["totals"][0] == b.n and got["totals"][4] == R.sum() and got["totals"][5] == 0
    assert (got["totals"][1:4] == got["counts"][:, 1:4].sum(axis=0)).all()
    assert (OL.words(got["ref_entries"]) != OL.POISON).all() and (got["ref_entries"]["d2"].view(np.uint32) == 0).all(), "every slot written, the distance word +0.0"
    ro, re_ = got["ref_offsets"], got["ref_entries"]
    assert (np.diff(ro) == R).all()
    owner = np.repeat(np.arange(b.n), R)
    pairs = np.unique(owner.astype(np.int64) * tris.shape[0] + re_["id"])
    assert (pairs == np.repeat(np.arange(b.n), m).astype(np.int64) * tris.shape[0] + want["ids"]).all(), "the ids among the references are the list"
    assert (re_["id"] >= b.firsts()[owner]).all()
    print(shape, name, "duplicate factor", R.sum() / max(1, m.sum()), "longest run of references", int(R.max()))
    if shape == "contact":
        assert (R >= 2).sum() >= 100
    else:
        assert (R > OL.SORT_CAP).sum() >= 8 and ((R > 64) & (R <= OL.SORT_CAP)).sum() > 100
    assert (R <= 1).sum() > 100


@pytest.mark.parametrize("name", OL.SCENES)
@pytest.mark.parametrize("shape", ["contact", "obb"])
def test_labelled_variants(fixtures, scenes, host, shape, name):
    """the labelled queries of the fixtures (`*_lab_*`): the walk through the protocol == the brute force == the fixture == the statement; labels of -1 skip
    nothing"""
    exe, d = host
    tris = scenes[name]
    b = OL.fixture_batch(shape, fixtures[shape], name, tris, labelled=True)
    arrays = oracle_arrays(scenes, name, True, True)
    got = OL.host_lists(exe, d, arrays, tris, b)
    want = brute(fixtures, scenes, host, shape, name, labelled=True)
    OL.assert_csr_equal(got, want, f"{shape} {name}: the labelled walk against the brute force")
    OL.assert_fixture(want, fixtures[shape], name + "_lab", f"{shape} {name}: the labelled brute force")
    OL.assert_csr_equal(b.statement(tris), want, f"{shape} {name}: the labelled statement")
    plain = brute(fixtures, scenes, host, shape, name)
    assert plain["ids"].size > want["ids"].size > 0
    minus = b.with_labels(np.full_like(np.asarray(b.query_labels), -1), b.tri_labels)
    OL.assert_csr_equal(OL.host_lists(exe, d, arrays, tris, minus), plain, f"{shape} {name}: labels of -1 skip nothing")


@pytest.mark.parametrize("name", OL.SCENES)
@pytest.mark.parametrize("shape", OL.SHAPES)
def test_paged_queries_continue_their_twins(fixtures, scenes, host, shape, name):
    """a PAGED query repeats another with first > 0: its list is the twin's list from `first` on"""
    tris = scenes[name]
    b = OL.fixture_batch(shape, fixtures[shape], name, tris)
    want = brute(fixtures, scenes, host, shape, name)
    sec, twin_from = OL.PAGED[shape]
    firsts = b.firsts()
    cut = 0
    for i in range(sec.start, sec.stop):
        twin = twin_from + (i - sec.start)
        mine = want["ids"][want["offsets"][i]:want["offsets"][i + 1]]
        theirs = want["ids"][want["offsets"][twin]:want["offsets"][twin + 1]]
        assert firsts[twin] == 0 and (mine == theirs[theirs >= firsts[i]]).all(), i
        cut += int(firsts[i] > 0 and mine.size < theirs.size)
    assert cut >= 32, "paged queries that leave something out"


@pytest.mark.parametrize("name", D.WALKED)
def test_deep_grids_at_every_stage(host, san_host, name):
    """every scene and stage of _deep_grids.CATALOGUE, the three shapes: the protocol on the host against the host brute force; once more with the stand-alone
    sanitizer build of the host program (brute force, walk, network, compact)"""
    exe, d = host
    tris = D.make_tris(name)
    gb = scene.grid_box(tris)
    batches = OL.deep_batches(name, tris)
    wants = [OL.host_brute(exe, d, tris, b, grid=gb) for b in batches]
    for b, w in zip(batches, wants):
        assert (np.diff(w["offsets"]) >= 2).sum() >= 16, b.shape
    OL.assert_csr_equal(OL.host_brute(san_host[0], san_host[1], tris, batches[2], grid=gb), wants[2], f"{name}: the sanitized brute force")
    st = D.OracleStages(name, tris)
    for stage in D.stages_of(name):
        out = D.stage_grid(st, stage)
        G = out[0] if stage == "compress" else out
        arrays = _host.oracle_grid_arrays(G)
        assert np.array_equal(np.float32(arrays["bbox_min"]), gb[0]) and np.array_equal(np.float32(arrays["bbox_max"]), gb[1])
        for b, w in zip(batches, wants):
            for which, (e, dd) in (("plain", host), ("san", san_host)):
                OL.assert_csr_equal(OL.host_lists(e, dd, arrays, tris, b), w, f"{name} {b.shape} after {stage} ({which})")


# ---- the library -------------------------------------------------------------------------------------------------------------------------

def test_kernel_resources_and_budget(fixtures):
    """tools/kernel_resources.py: no scratch and no spill for the new kernel, VGPRs and wavefronts per SIMD as found -- fewer registers than either k-list
    sibling; the pinned rows of overlap.hip as they were; tools/count_kernels.py: at most 120 kernels, the new kernel once, exactly one expand_select"""
    rows = _host.kernel_rows("overlap_lists")
    assert set(rows) == {"overlap_refs_kernel"}, rows
    assert rows["overlap_refs_kernel"] == (105, 0, 0, 4), rows
    rows = _host.kernel_rows("overlap")
    assert rows["obb_tris_kernel"] == (126, 0, 0, 4) and rows["overlap_boxes_kernel"] == (128, 0, 0, 4), rows
    c = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "count_kernels.py"), "-v"], capture_output=True, text=True, cwd=ROOT)
    m = re.search(r"(\d+) kernels", c.stdout)
    assert m and int(m.group(1)) <= 120, c.stdout[-300:] + c.stderr[-300:]
    assert c.stdout.count("overlap_refs_kernel") == 1
    assert c.stdout.count("expand_select") == 1, "the three axes of expand_select are one kernel"


def test_entry_points_and_no_allocation_site(fixtures):
    """the three symbols declared in the header, exported by the library (nm -D) and bound; ABI 3; the Python layer; overlap_lists.hip asks for no memory"""
    from hagrid_amd import api, lib
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "hagrid_amd.h")).read(), flags=re.S)
    assert re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", code)
    L = lib.load()
    assert L.hagrid_abi_version() == lib.ABI_VERSION == 3
    exported = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, nargs in (("hagrid_box_refs", 11), ("hagrid_tri_refs", 14), ("hagrid_obb_refs", 13)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert re.search(r"\sT\s+" + name + r"$", exported, flags=re.M), name
        assert name in lib.SIGNATURES and hasattr(L, name) and len(lib.SIGNATURES[name][1]) == nargs, name
    for name in ("box_refs", "tri_refs", "obb_refs", "box_lists", "contact_lists", "obb_lists"):
        assert hasattr(api, name) and name in api.__all__, name
    for name in ("box_lists", "contact_lists", "obb_lists"):
        assert hasattr(scene, name)
    one = np.zeros((1, 3), np.int32)                      # one label array without the other is refused in the Python layer as the entry points refuse it
    for call in (lambda **kw: api.obb_lists(api.Grid(), 0, np.zeros((1, 16), np.float32), **kw), lambda **kw: api.contact_lists(api.Grid(), 0, np.zeros((1, 12), np.float32), **kw)):
        for kw in ({"query_labels": one}, {"tri_labels": one}):
            with pytest.raises(api.HagridError, match="together"):
                call(**kw)
    prog = '#include "hagrid_amd.h"\nint main(void) { return sizeof(&hagrid_box_refs) + sizeof(&hagrid_tri_refs) + sizeof(&hagrid_obb_refs) ? 0 : 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-fsyntax-only", "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    source = open(os.path.join(ROOT, "hagrid_amd", "csrc", "overlap_lists.hip")).read()
    for site in ("pool_alloc<", "pool_try_alloc<", ".get<", "ctx_scan<", "scan_plain(", "hagrid_mem_alloc(", "device_request(", "lookback_state(", "hipMalloc"):
        assert site not in source, site
    header = open(os.path.join(INC, "hagrid", "overlap.h")).read()
    assert "NOT offered" not in header and "struct RefList" in header
