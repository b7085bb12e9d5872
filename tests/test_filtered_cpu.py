"""Filtered traversal (hagrid_traverse_grid_filtered), the part that needs no GPU: the numpy statement scene.filtered_hits against the reference-pinned
multi-hit fixture with the filter laid over its eight slots; the host walk tests/cpp/filtered_host.cpp -- the visitor of the gfx950 kernel over the same
HitList and RayFilter -- against that statement, every ray, every null combination, any-hit, once under the sanitizers; the "deleted triangles" identity;
and the entry point in header, library, bindings and shim."""
import os
import re
import subprocess

import numpy as np
import pytest

import _filtered as F
import _multi_hit as M
from hagrid_amd import scene

ROOT, INC = M.ROOT, M.INC


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def host(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("filtered_host")
    return F.build_host(d), d


@pytest.mark.parametrize("scene_name", F.SCENES)
def test_statement_against_the_fixture(built, scene_name):
    """scene.filtered_hits equals the filter applied to the fixture's eight slots on every DECIDED ray, ids and t bits; the rays left out are rays whose
    fixture list is full (measured with these generators: 29 / 31 / 46 / 79 soup rays and 1 / 1 / 3 / 7 mesh rays at k = 1 / 2 / 4 / 8)"""
    c = F.inputs(scene_name)
    F.assert_filter_bites(c)
    ids, t = F.wanted(scene_name, "both")
    full = (c.ids >= 0).all(axis=1)
    for k in (1, 2, 4, 8):
        f_ids, f_t, decided = F.from_fixture(c, k, c.filters, c.tri_masks)
        undecided = int((~decided).sum())
        print(f"{scene_name} k={k}: {undecided} rays undecided by the fixture")
        assert undecided <= F.UNDECIDED_CAP[scene_name] and (full[~decided]).all()
        bad = F.lists_differ(ids[:, :k], t[:, :k], f_ids, f_t) & decided
        assert not bad.any(), f"{scene_name} k={k}: {bad.sum()} decided rays differ, first at {np.flatnonzero(bad)[:5]}"
    # without any filter the statement is the fixture itself
    u_ids, u_t = F.wanted(scene_name, "neither")
    assert not F.lists_differ(u_ids, u_t, c.ids, c.t).any()
    # what the generators do to the lists: hits removed by skip, hits removed by the masks
    rows = np.repeat(np.arange(c.n), 8).reshape(c.n, 8)
    used = c.ids >= 0
    tri = np.where(used, c.ids, 0)
    by_skip = (used & ~scene.takes_part(rows, tri, c.filters, None)).any(axis=1).sum()
    by_mask = (used & ~scene.takes_part(rows, tri, np.stack([c.filters[:, 0], np.full(c.n, -1, np.int32)], axis=1), c.tri_masks)).any(axis=1).sum()
    assert by_skip > 500 and by_mask > 1000


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", F.SCENES)
def test_host_walk_against_the_statement(host, scene_name, compress):
    """all 4096 rays, k = 1, 2, 4, 8, over Cell and SmallCell grids of the CPU oracle, no ray excepted; the four null combinations; any-hit"""
    from oracle import oracle as O
    exe, d = host
    c = F.inputs(scene_name)
    G = O.Grid.full(c.tris, compress=compress)
    assert (G.small_cells is not None) == compress
    arrays = M.oracle_grid_arrays(G)
    for combo in F.COMBOS:
        f, m = F.combo_args(c, combo)
        ids, t = F.wanted(scene_name, combo)
        for k in (1, 2, 4, 8) if combo == "both" else (1, 8):
            got = F.host_walk(exe, d, arrays, c.tris, c.rays, k, f, m)
            F.assert_lists(got, ids, t, f"{scene_name} compress={compress} {combo} k={k}")
            assert (got["u"] == 0).all() and (got["v"] == 0).all()
        got = F.host_walk(exe, d, arrays, c.tris, c.rays, 1, f, m, any_hit=True)
        F.assert_any_hit(got, c.tris, c.rays, f, m, ids[:, 0], f"{scene_name} compress={compress} {combo} any-hit")
    # rays with mask 0 get k empty slots
    none = (c.filters[:, 0] == 0)
    ids, t = F.wanted(scene_name, "both")
    assert none.sum() > 500 and (ids[none] == -1).all() and (M.bits(t[none]) == M.bits(np.repeat(c.rays[none, 7:8], 8, axis=1))).all()


def test_host_walk_under_the_sanitizers(tmp_path, built):
    """one run of the stand-alone sanitized build on a 512-ray slice: lists and any-hit"""
    from oracle import oracle as O
    exe = F.build_host(tmp_path, sanitize=True)
    c = F.inputs("soup")
    arrays = M.oracle_grid_arrays(O.Grid.full(c.tris, compress=True))
    sl = slice(2048, 2560)                          # the end of the primary rays and the start of the incoherent ones
    ids, t = F.wanted("soup", "both")
    got = F.host_walk(exe, tmp_path, arrays, c.tris, c.rays[sl], 8, c.filters[sl], c.tri_masks)
    F.assert_lists(got, ids[sl], t[sl], "soup, sanitized host walk")
    got = F.host_walk(exe, tmp_path, arrays, c.tris, c.rays[sl], 1, c.filters[sl], c.tri_masks, any_hit=True)
    F.assert_any_hit(got, c.tris, c.rays[sl], c.filters[sl], c.tri_masks, ids[sl, 0], "soup, sanitized host walk, any-hit")


@pytest.mark.parametrize("mask", [0x06, 0x15])
def test_deleted_triangles_identity(built, mask):
    """for one ray mask: filtered_hits equals the unfiltered lists over tris[take_part], ids mapped back"""
    c = F.inputs("soup")
    rays = c.rays[:1024]
    f = np.empty((rays.shape[0], 2), dtype=np.int32); f[:, 0] = mask; f[:, 1] = -1
    part = np.flatnonzero((c.tri_masks & np.uint32(mask)) != 0)
    assert 0 < part.size < c.num_tris
    ids, t = scene.filtered_hits(c.tris, rays, 8, f, c.tri_masks)
    sub_ids, sub_t = scene.filtered_hits(c.tris[part], rays, 8)
    back = np.where(sub_ids >= 0, part[np.where(sub_ids >= 0, sub_ids, 0)], -1)
    assert (ids == back).all() and (M.bits(t) == M.bits(sub_t)).all()
    assert (ids[:, 0] >= 0).sum() > 100 and (ids[:, 0] != c.ids[:1024, 0]).any()


def test_takes_part_rules():
    """any negative skip skips nothing, a skip that names no triangle skips nothing, the mask is read as 32 bits"""
    f = np.array([[-1, -1], [-1, -5], [-1, 3], [-1, 1 << 30], [0, -1], [np.int32(-2147483648), -1], [2, -2147483648]], dtype=np.int32)
    masks = np.array([1, 2, 0x80000000, 0xFFFFFFFF, 0], dtype=np.uint32)
    r, j = np.meshgrid(np.arange(7), np.arange(5), indexing="ij")
    got = scene.takes_part(r.reshape(-1), j.reshape(-1), f, masks).reshape(7, 5)
    assert got.tolist() == [[True, True, True, True, False], [True, True, True, True, False], [True, True, True, False, False], [True, True, True, True, False],
                            [False] * 5, [False, False, True, True, False], [False, True, False, True, False]]
    assert scene.takes_part(r.reshape(-1), j.reshape(-1), None, None).all()


def test_entry_point_declared_exported_and_bound(built):
    from hagrid_amd import api, lib
    header = open(os.path.join(INC, "hagrid_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"#define\s+HAGRID_RAY_MASK_ALL\s+0xFFFFFFFFu\b", code) and re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", code)
    assert re.search(r"\bint\s+hagrid_traverse_grid_filtered\s*\(", code)
    L = lib.load()
    assert "hagrid_traverse_grid_filtered" in lib.SIGNATURES and hasattr(L, "hagrid_traverse_grid_filtered")
    assert len(lib.SIGNATURES["hagrid_traverse_grid_filtered"][1]) == 10
    for name in ("traverse_grid_filtered", "skip_filters", "RAY_MASK_ALL", "MeshScene"):
        assert hasattr(api, name) and name in api.__all__, name
    assert api.RAY_MASK_ALL == 0xFFFFFFFF == scene.RAY_MASK_ALL and hasattr(api.MeshScene, "instance_masks")
    assert "traverse_grid_filtered" in open(os.path.join(INC, "hagrid", "traverse.h")).read()
    prog = ('#include "hagrid_amd.h"\nint main(void) { return HAGRID_RAY_MASK_ALL == 0xFFFFFFFFu && sizeof(&hagrid_traverse_grid_filtered) ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-fsyntax-only", "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ray_filter_header_is_cxx11(tmp_path):
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-DHOST=", "-DDEVICE=", "-I", INC, "-fsyntax-only", "-x", "c++",
                        os.path.join(INC, "hagrid", "ray_filter.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = tmp_path / "f.cpp"
    src.write_text(r'''
#include <cstdio>
#include "hagrid/ray_filter.h"
using namespace hagrid;
int main() {
    const uint32_t masks[3] = {1u, 0x80000000u, 0u};
    const RayFilter all, f(0x80000001u, 1), none(0u, -1), rec[2] = {RayFilter(2u, -7), RayFilter(1u, 2)};
    printf("%d%d%d ", int(all.walks()), int(all.skips(0)), int(all.admits(nullptr, 5)));
    printf("%d%d%d%d%d ", int(f.skips(1)), int(f.skips(0)), int(f.admits(masks, 0)), int(f.admits(masks, 1)), int(f.admits(masks, 2)));
    printf("%d%d ", int(none.walks()), int(none.admits(nullptr, 0)));
    printf("%d %d %d\n", RayFilter::of(rec, 1).skip, RayFilter::of(nullptr, 1).skip, int(RayFilter::of(rec, 0).skips(0)));
    return 0;
}''')
    exe = str(tmp_path / "f")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-DHOST=", "-DDEVICE=", "-I", INC, str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "101 10110 00 2 -1 0"
