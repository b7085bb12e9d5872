"""Crossing lists (hagrid_list_crossings), the part that needs no GPU: the fixture tests/golden/crossing_lists.npz (accept and t of every pair by the
reference's arithmetic, the facing by numpy) against scene.ray_crossing_lists, crossings.npz and multi_hit.npz; the host program
tests/cpp/crossing_lists_host.cpp -- the brute force and the walk of include/hagrid/crossings.h with an array sink, the walk and the slot rules the gfx950
kernel runs -- against the fixture, every bit, for page capacities 1, 2, 3, 4 and 8 over Cell and SmallCell grids of both expansion modes; what every slot
holds for rooms that are too short, too long and malformed (scene.crossing_slots); hostile rays; the sink by itself; the program under AddressSanitizer and
UBSan."""
import subprocess

import numpy as np
import pytest

import _crossing_lists as CL
import _crossings as X
import _multi_hit as M
from hagrid_amd import scene

INC = X.INC


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return {**np.load(X.FIXTURE), **np.load(CL.FIXTURE)}


@pytest.fixture(scope="module")
def scenes():
    return {s: X.make_tris(s) for s in X.SCENES}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("crossing_lists_host")
    return CL.build_host(d), d


def test_fixture_shape(fixture):
    import os
    assert os.path.getsize(CL.FIXTURE) < 1000000
    totals = {"soup": 7253, "mesh": 4728, "solids": 1293}
    for s in X.SCENES:
        o, t, key = CL.fixture_lists(fixture, s)
        rec = fixture[s + "_records"]
        assert o.dtype == np.int64 and fixture[s + "_t"].dtype == np.uint32 and key.dtype == np.int32
        assert o[0] == 0 and o[-1] == totals[s] == t.size == key.size
        m = o[1:] - o[:-1]
        assert (m == rec[:, 0].view(np.int32)).all(), "the lengths are the counts of crossings.npz"
        assert m.max() <= 28 and (m > 9).any(), "the strides of the slot tests stand below, at and above the page and above the longest list"
        ray = np.repeat(np.arange(m.size), m)
        same = ray[1:] == ray[:-1]
        assert (((t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & (key[1:] >> 1 > key[:-1] >> 1)))[same]).all(), "strictly increasing in (t, id) inside a ray"
        has = m > 0
        assert (M.bits(t[o[:-1][has]]) == rec[has, 1]).all(), "the first entry is the record's t_first"
        assert (key >= 0).all() and (key >> 1 < X.make_tris(s).shape[0]).all()


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_fixture_equals_numpy(fixture, scenes, scene_name):
    """scene.ray_crossing_lists, every bit; the records from the lists (records_from_pairs) are crossings.npz; scene.ray_crossings is unchanged"""
    rays = fixture[scene_name + "_rays"]
    o, t, key = CL.fixture_lists(fixture, scene_name)
    mo, mt, mk = scene.ray_crossing_lists(scenes[scene_name], rays)
    assert mo.dtype == np.int64 and mt.dtype == np.float32 and mk.dtype == np.int32
    assert (mo == o).all() and (M.bits(mt) == M.bits(t)).all() and (mk == key).all()
    ray = np.repeat(np.arange(rays.shape[0]), o[1:] - o[:-1])
    X.assert_records_equal(X.records_from_pairs(rays, ray, key >> 1, t, (key & 1) != 0), fixture[scene_name + "_records"], scene_name + ": records from the lists")
    X.assert_records_equal(scene.ray_crossings(scenes[scene_name], rays), fixture[scene_name + "_records"], scene_name + ": ray_crossings")


@pytest.mark.parametrize("scene_name", M.SCENES)
def test_fixture_agrees_with_multi_hit(fixture, scene_name):
    """the first min(m, 8) entries of every ray are multi_hit.npz in id and t"""
    mh = np.load(M.FIXTURE)
    ids, ts = mh[scene_name + "_ids"], M.bits(mh[scene_name + "_t"])
    o, t, key = CL.fixture_lists(fixture, scene_name)
    slots = scene.crossing_slots(8, 8 * (o.size - 1), (o, t, key), fixture[scene_name + "_rays"][:, 7])
    n = ids.shape[0]
    k = slots["key"].reshape(-1, 8)[:n]
    assert (np.where(k >= 0, k >> 1, -1) == ids).all()
    assert (slots["t"].reshape(-1, 8)[:n][k >= 0] == ts[k >= 0]).all()


def test_crossing_slots_by_hand():
    """scene.crossing_slots on three rays written out: a list that fits exactly, one cut short, one padded; a malformed pair owns nothing"""
    lists = (np.int64([0, 2, 5, 5]), np.float32([1, 2, 3, 4, 5]), np.int32([10, 21, 30, 41, 50]))
    tmax = np.float32([9, np.inf, 7])
    inf = int(np.float32(np.inf).view(np.uint32)); f = lambda v: int(np.float32(v).view(np.uint32))
    s = scene.crossing_slots(np.int64([0, 2, 4, 6]), 6, lists, tmax)
    assert s["key"].tolist() == [10, 21, 30, 41, -1, -1] and s["t"].tolist() == [f(1), f(2), f(3), f(4), f(7), f(7)] and s["written"].all()
    assert (s["count"], s["short"]) == (4, 1)
    s = scene.crossing_slots(2, 7, lists, tmax)
    assert s["key"].tolist() == [10, 21, 30, 41, -1, -1, 0] and s["written"].tolist() == [True] * 6 + [False]
    s = scene.crossing_slots(np.int64([0, 3, 2, 8]), 7, lists, tmax)          # ray 1 decreasing, ray 2 beyond the capacity
    assert s["key"].tolist() == [10, 21, -1, 0, 0, 0, 0] and s["t"][2] == f(9) and s["written"].tolist() == [True] * 3 + [False] * 4
    assert (s["count"], s["short"]) == (2, 1)
    s = scene.crossing_slots(np.int64([-1, 2, 5, 5]), 5, lists, tmax)         # ray 0 negative
    assert s["written"].tolist() == [False, False, True, True, True] and s["t"][4] == f(5) and inf != f(5)


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_host_brute_force_reproduces_the_fixture(fixture, scenes, host, scene_name):
    exe, d = host
    lists = CL.fixture_lists(fixture, scene_name)
    rays = fixture[scene_name + "_rays"]
    got = CL.host_lists(exe, d, scenes[scene_name], rays, int(lists[0][-1]), offsets=lists[0])
    want = scene.crossing_slots(lists[0], int(lists[0][-1]), lists, rays[:, 7])
    assert want["written"].all() and (want["key"] >= 0).all(), "offsets from the counts: every slot written once, no empty entry"
    CL.assert_slots(got, want, scene_name)
    X.assert_records_equal(got["records"], fixture[scene_name + "_records"], scene_name)


@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", X.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, scenes, host, scene_name, compress, subset_only):
    """every entry and every record equal, no ray excepted, for page capacities 1, 2, 3, 4 and 8; flushes within ceil(m / P) + 1"""
    exe, d = host
    tris = scenes[scene_name]
    G = X.oracle_grid(tris, compress, subset_only)
    assert (G.small_cells is not None) == compress
    arrays = X.oracle_grid_arrays(G)
    rays = fixture[scene_name + "_rays"]
    lists = CL.fixture_lists(fixture, scene_name)
    total = int(lists[0][-1])
    want = scene.crossing_slots(lists[0], total, lists, rays[:, 7])
    for page in X.PAGES:
        got = CL.host_lists(exe, d, tris, rays, total, offsets=lists[0], grid=arrays, page=page)
        what = f"{scene_name} compress={compress} subset_only={subset_only} P={page}"
        CL.assert_slots(got, want, what)
        X.assert_records_equal(got["records"], fixture[scene_name + "_records"], what)
        assert got["excess"] <= 0, f"P={page}: a ray flushed {got['excess']} times more than ceil(m / P) + 1"
        assert got["totals"][0] == rays.shape[0] and got["totals"][3] > 0 and got["totals"][4] == total and got["totals"][5] == 0


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_slots_in_stride_form(fixture, scenes, host, scene_name):
    """S = 1, 3, 8, 9, 32: the first min(m, S) entries, then empty entries; the list for S is a prefix of the list for the next S; records do not depend on S"""
    exe, d = host
    tris = scenes[scene_name]
    arrays = X.oracle_grid_arrays(X.oracle_grid(tris, True, True))
    rays = fixture[scene_name + "_rays"]
    n = rays.shape[0]
    lists = CL.fixture_lists(fixture, scene_name)
    prev = None
    for S in CL.STRIDES:
        cap = n * S + 3                     # three slots nobody owns
        want = scene.crossing_slots(S, cap, lists, rays[:, 7])
        for grid, page in ((arrays, 8), (arrays, 3), (None, 8)):
            got = CL.host_lists(exe, d, tris, rays, cap, stride=S, grid=grid, page=page)
            CL.assert_slots(got, want, f"{scene_name} S={S} P={page} walk={grid is not None}")
            X.assert_records_equal(got["records"], fixture[scene_name + "_records"], f"{scene_name} S={S}")
        if prev is not None:
            k0, t0, S0 = prev
            # what the shorter room got is a prefix of what the longer room gets, pads included
            assert (got["key"][:n * S].reshape(n, S)[:, :S0] == k0).all() and (got["t"][:n * S].reshape(n, S)[:, :S0] == t0).all()
        prev = (got["key"][:n * S].reshape(n, S).copy(), got["t"][:n * S].reshape(n, S).copy(), S)
    assert want["count"] == lists[0][-1] and want["short"] == 0, "S = 32 holds every list whole"


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_slots_in_csr_form(fixture, scenes, host, scene_name):
    """exact offsets, every room one short, every room two long, and a negative, a decreasing and a beyond-capacity pair, which write nothing"""
    exe, d = host
    tris = scenes[scene_name]
    arrays = X.oracle_grid_arrays(X.oracle_grid(tris, False, True))
    rays = fixture[scene_name + "_rays"]
    lists = CL.fixture_lists(fixture, scene_name)
    for name, offsets, cap in CL.layouts(lists):
        want = scene.crossing_slots(offsets, cap, lists, rays[:, 7])
        if name == "malformed":
            m = lists[0][1:] - lists[0][:-1]
            assert not want["written"].all() and want["short"] == int((m[[2, 3, -1]] > 0).sum()) and m[-1] > 0
        for grid, page in ((arrays, 8), (arrays, 2), (None, 8)):
            got = CL.host_lists(exe, d, tris, rays, cap, offsets=offsets, grid=grid, page=page)
            CL.assert_slots(got, want, f"{scene_name} {name} P={page} walk={grid is not None}")
            X.assert_records_equal(got["records"], fixture[scene_name + "_records"], f"{scene_name} {name}: the records do not depend on the rooms")


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", ["soup", "mesh"])
def test_hostile_rays_through_the_host_walk(scenes, host, scene_name, compress):
    """the catalogue of tests/_hostile_rays.py, lists against the header's brute force with the same sink under the contract of X.assert_hostile_records: the
    strict families bit for bit, every entry; (i) and (l) held to termination and the flush bound; (k) within H.AMBIGUOUS_CAP (measured: DESIGN.md 4.9)"""
    import _hostile_rays as H
    exe, d = host
    tris = scenes[scene_name]
    G = X.oracle_grid(tris, compress, True)
    rays, family = H.catalogue(tris, G, mesh=scene_name == "mesh")
    first = CL.host_lists(exe, d, tris, rays, 0, stride=0, offsets=np.zeros(rays.shape[0] + 1, np.int64))          # no room at all: the records alone
    counts = first["records"]["id"].astype(np.int64)
    assert first["totals"][4] == 0 and first["totals"][5] == (counts > 0).sum()
    offsets = np.zeros(rays.shape[0] + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[-1])
    want = CL.host_lists(exe, d, tris, rays, total, offsets=offsets)
    X.assert_records_equal(want["records"], first["records"], "the records do not depend on the rooms")
    assert (want["key"] >= 0).all() and (want["guard"] == CL.POISON).all()
    strict = ~np.isin(family, ["i", "k", "l"])
    k = family == "k"
    for page in (1, 8):
        got = CL.host_lists(exe, d, tris, rays, total, offsets=offsets, grid=X.oracle_grid_arrays(G), page=page)
        X.assert_hostile_records(got["records"], want["records"], family, f"P={page}")
        bad = CL.rays_that_differ(got, want, offsets)
        print(f"{scene_name} compress={compress} P={page}: {(bad & k).sum()} of {k.sum()} rays of family (k) differ in record or list, {(bad & ~strict & ~k).sum()} of (i), (l)")
        assert not (bad & strict).any(), f"P={page}: {(bad & strict).sum()} rays differ, families {sorted(set(family[bad & strict]))}, first at {np.flatnonzero(bad & strict)[:5]}"
        assert (bad & k).sum() <= H.AMBIGUOUS_CAP * k.sum(), f"P={page}: {(bad & k).sum()} of {k.sum()} rays of family (k) differ"
        assert got["excess"] <= 0 and (got["guard"] == CL.POISON).all()
    refused = ~H._admissible(rays)
    assert refused.any() and (counts[refused] == 0).all()
    # inadmissible and inactive rays with room: empty entries with the bits of their tmax
    sel = np.flatnonzero(refused)[:64]
    r = np.concatenate([rays[sel], rays[:2]]); r[-1, 7] = -1.0
    got = CL.host_lists(exe, d, tris, r, 2 * r.shape[0], stride=2, grid=X.oracle_grid_arrays(G))
    assert (got["key"].reshape(-1, 2)[:sel.size] == -1).all() and (got["key"][-2:] == -1).all()
    assert (got["t"].reshape(-1, 2)[:sel.size] == M.bits(r[:sel.size, 7])[:, None]).all() and (got["t"][-2:] == M.bits(np.float32(-1.0))).all()


def test_sink_rules(tmp_path):
    """Page::flush with a sink: called once per folded entry, in order, with the count before the fold as the position -- across two pages; without a sink as before"""
    src = tmp_path / "sink.cpp"
    src.write_text(r'''
#include <cstdio>
#include "hagrid/crossings.h"
using namespace hagrid;
using namespace hagrid::crossings;
struct Print { void operator()(int position, float t, uint32_t key) const { printf("%d:%g:%u ", position, t, key); } };
int main() {
    Page<4> p; Accum a;
    p.init(3); a.init(9.0f);
    p.insert(5.0f, 7u << 1); p.insert(5.0f, 3u << 1 | 1u); p.insert(6.5f, 1u << 1); p.insert(6.0f, 0u << 1 | 1u);
    p.flush(a, Print());
    p.insert(5.0f, 7u << 1); p.insert(6.5f, 1u << 1); p.insert(8.5f, 4u << 1);
    p.flush(a, Print());
    printf("\n%d %d\n", a.count, a.winding);
    p.insert(9.0f, 2u << 1);
    p.flush(a);
    printf("%d\n", a.count);
    long long first, room;
    const long long o[4] = {0, 4, 2, 9};
    for (int i = 0; i < 3; i++) { slot_range(o, 0, 8, i, first, room); printf("%lld+%lld ", first, room); }
    slot_range(nullptr, 5, 100, 3, first, room); printf("%lld+%lld\n", first, room);
    return 0;
}''')
    exe = str(tmp_path / "sink")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC, str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == ["0:5:7", "1:5:14", "2:6:1", "3:6.5:2", "4:8.5:8"]
    assert out[1] == "5 1" and out[2] == "6"
    assert out[3] == "0+4 0+0 0+0 15+5"            # a decreasing pair and one beyond the capacity have no room


def test_host_program_under_sanitizers(fixture, scenes, tmp_path):
    """the host program with -fsanitize=address,undefined, once, as a stand-alone binary on the soup: brute force and walk, rooms short, long and malformed"""
    exe = CL.build_host(tmp_path, sanitize=True)
    tris = scenes["soup"]
    rays = fixture["soup_rays"]
    sel = np.r_[0:256, rays.shape[0] - 64:rays.shape[0]]             # primary rays and the aimed ones with many crossings
    o, t, key = CL.fixture_lists(fixture, "soup")
    m = (o[1:] - o[:-1])[sel]
    so = np.zeros(sel.size + 1, np.int64); np.cumsum(m, out=so[1:])
    idx = np.concatenate([np.arange(o[i], o[i + 1]) for i in sel]) if so[-1] else np.zeros(0, np.int64)
    lists = (so, t[idx], key[idx])
    arrays = X.oracle_grid_arrays(X.oracle_grid(tris, True, True))
    for name, offsets, cap in CL.layouts(lists):
        got = CL.host_lists(exe, tmp_path, tris, rays[sel], cap, offsets=offsets, grid=arrays, page=3)
        CL.assert_slots(got, scene.crossing_slots(offsets, cap, lists, rays[sel, 7]), "sanitized walk, " + name)
        X.assert_records_equal(got["records"], fixture["soup_records"][sel], "sanitized walk")
    got = CL.host_lists(exe, tmp_path, tris, rays[sel[-16:]], 16 * 9, stride=9)
    sub = (so[-17:] - so[-17], lists[1][so[-17]:], lists[2][so[-17]:])
    CL.assert_slots(got, scene.crossing_slots(9, 16 * 9, sub, rays[sel[-16:], 7]), "sanitized brute force, S = 9")
