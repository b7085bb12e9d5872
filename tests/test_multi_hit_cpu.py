"""Multi-hit traversal, the part that needs no GPU: the fixture tests/golden/multi_hit.npz (the 8 nearest intersections of every ray by
the reference's arithmetic) against the live oracle; the host walk tests/cpp/multi_hit_host.cpp -- the walk of the gfx950 kernel, over
the same HitList of include/hagrid/multi_hit.h -- against the fixture, exactly; the new entry points in header, library and bindings;
and the layered picture: shade_layers of include/hagrid/frame.h against hagrid_amd/scene.py byte for byte."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _multi_hit as M

ROOT = M.ROOT
INC = M.INC


@pytest.fixture(scope="module")
def fixture():
    import __graft_entry__ as g
    g.build()
    return np.load(M.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("multi_hit_host")
    return M.build_host(d), d


def test_fixture_shape_and_order(fixture):
    want_hist = {"soup": [1670, 745, 544, 353, 303, 197, 128, 73, 83], "mesh": [945, 2451, 239, 362, 59, 20, 12, 1, 7]}
    for s in M.SCENES:
        rays, ids, t = fixture[s + "_rays"], fixture[s + "_ids"], fixture[s + "_t"]
        assert rays.shape == (4096, 8) and ids.shape == (4096, 8) and t.shape == (4096, 8)
        assert ids.dtype == np.int32 and t.dtype == np.float32 and rays.dtype == np.float32
        assert (M.bits(rays) == M.bits(M.fixture_rays(M.make_tris(s)))).all(), "the fixture's rays are the generators' rays"
        assert M.hit_histogram(ids) == want_hist[s]
        used = ids >= 0
        assert (used[:, 1:] <= used[:, :-1]).all(), "unused slots come last"
        assert (t[~used] == np.repeat(rays[:, 7:8], 8, axis=1)[~used]).all(), "unused slots hold the ray's tmax"
        pair = used[:, 1:]
        a_t, b_t, a_i, b_i = t[:, :-1][pair], t[:, 1:][pair], ids[:, :-1][pair], ids[:, 1:][pair]
        assert ((a_t < b_t) | ((a_t == b_t) & (a_i < b_i))).all(), "sorted by (t, id), no triangle twice"
        assert (t[used] >= np.repeat(rays[:, 3:4], 8, axis=1)[used]).all() and (t[used] <= np.repeat(rays[:, 7:8], 8, axis=1)[used]).all()
        assert os.path.getsize(M.FIXTURE) < 1000000


@pytest.mark.parametrize("scene_name", M.SCENES)
def test_fixture_against_the_live_oracle(fixture, scene_name):
    """a 256-ray slice, every triangle alone through the oracle's own intersect_prim_ray (this project's arithmetic, not the reference harness)"""
    tris = M.make_tris(scene_name)
    sl = slice(2200, 2456)                          # the end of the primary rays and the start of the incoherent ones
    ids, t = M.lists_by_brute_force(tris, fixture[scene_name + "_rays"][sl], use_ref=False)
    assert (ids == fixture[scene_name + "_ids"][sl]).all()
    assert (M.bits(t) == M.bits(fixture[scene_name + "_t"][sl])).all()
    assert (ids >= 0).any() and (ids < 0).any()


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("scene_name", M.SCENES)
def test_host_walk_reproduces_the_fixture(fixture, host, scene_name, compress):
    """ids equal, t bit-equal, no ray excepted, for k = 1, 2, 4, 8, over Cell and SmallCell grids of the CPU oracle"""
    from oracle import oracle as O
    exe, d = host
    tris = M.make_tris(scene_name)
    G = O.Grid.full(tris, compress=compress)
    assert (G.small_cells is not None) == compress
    arrays = M.oracle_grid_arrays(G)
    rays, ids, t = fixture[scene_name + "_rays"], fixture[scene_name + "_ids"], fixture[scene_name + "_t"]
    for k in (1, 2, 4, 8):
        got = M.host_walk(exe, d, arrays, tris, rays, k)
        bad = (got["id"] != ids[:, :k]).any(axis=1) | (M.bits(got["t"]) != M.bits(t[:, :k])).any(axis=1)
        assert not bad.any(), f"k={k}: {bad.sum()} of {bad.size} rays differ, first at {np.flatnonzero(bad)[:5]}"
        assert (got["u"] == 0).all() and (got["v"] == 0).all()


def test_hit_list_rules(tmp_path):
    """HitList by itself: duplicates kept once, ties in t resolved by id, a full list drops its last entry, slots beyond k stay empty"""
    src = tmp_path / "list.cpp"
    src.write_text(r'''
#include <cstdio>
#include "hagrid/multi_hit.h"
using namespace hagrid;
int main() {
    HitList<4> l;
    l.init(3, 9.0f);
    bool r[8];
    r[0] = l.insert(5.0f, 7, 0.1f, 0.2f);      // [7]
    r[1] = l.insert(5.0f, 7, 0.1f, 0.2f);      // duplicate
    r[2] = l.insert(5.0f, 3, 0.3f, 0.4f);      // tie in t: id 3 before id 7
    r[3] = l.insert(6.0f, 1, 0.0f, 0.0f);      // [3, 7, 1], full
    r[4] = l.insert(6.0f, 2, 0.0f, 0.0f);      // not before (6, 1)
    r[5] = l.insert(6.0f, 0, 0.5f, 0.6f);      // before (6, 1): [3, 7, 0]
    r[6] = l.insert(6.0f, 1, 0.0f, 0.0f);      // the dropped triangle comes again: refused
    r[7] = l.insert(1.0f, 9, 0.0f, 0.0f);      // [9, 3, 7]
    for (int i = 0; i < 8; i++) printf("%d", int(r[i]));
    printf("\n");
    for (int j = 0; j < 4; j++) printf("%d %g %g %g\n", l.id[j], l.t[j], l.u[j], l.v[j]);
    printf("%d %d %g\n", int(l.full()), l.last_id, l.last_t);
    return 0;
}''')
    exe = str(tmp_path / "list")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC, str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "10110101"
    assert out[1:5] == ["9 1 0 0", "3 5 0.3 0.4", "7 5 0.1 0.2", "-1 9 0 0"]
    assert out[5] == "1 7 5"


def test_multi_hit_header_is_cxx11():
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-DHOST=", "-DDEVICE=", "-I", INC, "-fsyntax-only", "-x", "c++",
                        os.path.join(INC, "hagrid", "multi_hit.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("multi_hit.h", "traverse.h"):
        assert not re.search(r'#\s*include\s*[<"][^>"]*frame\.h', open(os.path.join(INC, "hagrid", name)).read()), name


def test_entry_points_declared_exported_and_bound(fixture):
    from hagrid_amd import api, lib
    header = open(os.path.join(INC, "hagrid_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"#define\s+HAGRID_MAX_HITS\s+8\b", code) and re.search(r"#define\s+HAGRID_ABI_VERSION\s+3\b", code)
    L = lib.load()
    for name in ("hagrid_traverse_grid_multi", "hagrid_shade_layers"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in lib.SIGNATURES and hasattr(L, name)
    assert len(lib.SIGNATURES["hagrid_traverse_grid_multi"][1]) == 8 and len(lib.SIGNATURES["hagrid_shade_layers"][1]) == 7
    for name in ("traverse_grid_multi", "shade_layers", "MAX_HITS"):
        assert hasattr(api, name) and name in api.__all__
    assert api.MAX_HITS == 8
    assert "traverse_grid_multi" in open(os.path.join(INC, "hagrid", "traverse.h")).read()
    # the header still compiles as C99
    prog = '#include "hagrid_amd.h"\nint main(void) { return HAGRID_MAX_HITS == 8 && sizeof(&hagrid_traverse_grid_multi) && sizeof(&hagrid_shade_layers) ? 0 : 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-fsyntax-only", "-x", "c", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _layers_host(host, hits, k, clip, opacity):
    exe, d = host
    n = hits.size // k
    f_in, f_par, f_out = str(d / "layers_in.bin"), str(d / "layers_params.bin"), str(d / "layers_out.bin")
    np.ascontiguousarray(hits).tofile(f_in)
    with open(f_par, "wb") as f:
        f.write(struct.pack("<iffi", k, clip, opacity, n))
    subprocess.run([exe, "layers", f_par, f_in, f_out], check=True, timeout=300)
    return np.fromfile(f_out, dtype=np.uint8).reshape(n, 4)


def _random_lists(n, k, seed):
    """sorted random lists with 0 .. k entries, some t negative, some beyond any clip"""
    from hagrid_amd import scene
    rng = np.random.default_rng(seed)
    h = np.zeros((n, k), dtype=scene.HIT_DTYPE)
    count = rng.integers(0, k + 1, size=n)
    count[:4] = 0; count[4:8] = k
    t = np.sort(rng.uniform(-0.5, 3.5, size=(n, k)).astype(np.float32), axis=1)
    used = np.arange(k)[None, :] < count[:, None]
    h["id"] = np.where(used, rng.integers(0, 100000, size=(n, k)), -1)
    h["t"] = np.where(used, t, np.float32(7.0))
    return h


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("opacity", [1.0, 0.5, 0.3, 1e-3])
def test_shade_layers_host_function_against_scene(host, k, opacity):
    from hagrid_amd import scene
    h = _random_lists(5000, k, seed=11 + k)
    for clip in (2.5, 0.7):
        want = scene.shade_layers(h, k, clip, opacity)
        got = _layers_host(host, h, k, clip, opacity)
        assert want.shape == got.shape and (got == want).all(), np.flatnonzero((got != want).any(axis=1))[:5]
        assert (want[:, 3] == 255).all() and (want[:, 0] == want[:, 1]).all() and (want[:, 1] == want[:, 2]).all()
        assert (want[(h["id"] < 0).all(axis=1), 0] == 255).all(), "an empty list shades to white"


def test_shade_layers_opaque_is_the_depth_picture_of_slot_0(fixture):
    from hagrid_amd import scene
    for s in M.SCENES:
        rays, ids, t = fixture[s + "_rays"], fixture[s + "_ids"], fixture[s + "_t"]
        h = np.zeros(ids.shape, dtype=scene.HIT_DTYPE)
        h["id"] = ids; h["t"] = t
        clip = float(rays[1, 7])                    # a primary ray's tmax: the scene diagonal
        layered = scene.shade_layers(h, 8, clip, 1.0)
        depth = scene.shade_hits(np.ascontiguousarray(h[:, 0]), scene.SHADE_DEPTH, clip)
        same = (ids[:, 0] >= 0) | (rays[:, 7] >= np.float32(clip))
        assert same.sum() > 3000 and (layered[same] == depth[same]).all()
        assert (layered[ids[:, 0] < 0, 0] == 255).all()
    with pytest.raises(ValueError):
        scene.shade_layers(h, 8, 0.0, 0.5)
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError):
            scene.shade_layers(h, 8, 1.0, bad)
