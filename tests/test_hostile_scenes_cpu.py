"""The CPU oracle on the hostile-scene catalogues (tests/_hostile_scenes.py; DESIGN.md section 2, "Admissible scenes"): flat scenes build, pass the grid
check and answer rays as the brute force does; scenes with non-finite triangles, boxes that overflow, reference totals beyond 32 bits and depths beyond 23
levels are refused with the code that says which; a stand-alone program runs the construction of every catalogue under the sanitizers.  The kernels are
pinned to this oracle by tests/test_hostile_scenes_gpu.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import _hostile_rays as H
import _hostile_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT = S.flat_scenes()
ORC_ERANGE, ORC_ERANGE_LEVELS, ORC_EINVAL, ORC_ERANGE_BOX = -1, -2, -3, -4


def words(hits) -> np.ndarray:
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4)


def grid_arrays(G):
    return [np.array(G.entries), np.array(G.ref_ids), np.array(G.cells if G.cells is not None else G.small_cells), G.bbox_min, G.bbox_max,
            np.array(G.dims), np.array([G.shift]), np.array(G.offsets)]


def same_grid(A, B):
    return all(a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(grid_arrays(A), grid_arrays(B)))


def orc_build(tris, top=S.TOP_DENSITY, snd=S.SND_DENSITY):
    """(return code of orc_build_grid, the grid as the call left it)"""
    tris = np.ascontiguousarray(tris, np.float32)
    G = O.Grid()
    rc = O.lib().orc_build_grid(tris.ctypes.data_as(C.c_void_p), tris.shape[0], C.byref(G.g), top, snd)
    return rc, G


@functools.lru_cache(maxsize=None)
def _flat(name, compress):
    tris = FLAT[name]
    G = O.Grid.full(tris, compress=compress)
    rays, fam = S.scene_rays(tris, O.Grid.full(tris)) if compress else S.scene_rays(tris, G)
    return tris, G, rays, fam


@pytest.mark.parametrize("name", list(FLAT))
def test_flat_fixture_is_flat_and_recorded(name):
    """every fixture has an extent for which Cleary's formula is undefined, and builds the grid DESIGN.md section 2 records for it"""
    tris = FLAT[name]
    lo, hi = S.scene.tris_bbox(tris)
    bb = O.OBBox(); bb.min[:] = [float(x) for x in lo]; bb.max[:] = [float(x) for x in hi]
    assert not O.lib().orc_grid_dims_defined(C.byref(bb), tris.shape[0], S.TOP_DENSITY)
    rc, G = orc_build(tris)
    assert rc == 0
    print(name, tris.shape[0], G.dims, G.shift, G.num_cells, G.num_refs)
    assert (tuple(G.dims), G.shift, G.num_cells, G.num_refs) == S.RECORDED[name]
    # the widened box holds the scene, has a positive normal volume, and every plane pair of it is distinct
    e = G.bbox_max - G.bbox_min
    assert (G.bbox_min <= lo).all() and (G.bbox_max >= hi).all() and (e > 0).all() and np.prod(e, dtype=np.float32) >= np.finfo(np.float32).tiny
    assert G.num_refs > 0 or name == "point"


@pytest.mark.parametrize("compress", [False, True], ids=["cell", "small"])
@pytest.mark.parametrize("name", list(FLAT))
def test_flat_scene_builds_checks_and_answers_as_the_brute_force(name, compress):
    """Grid.full succeeds, Grid.check passes with coverage, the construction and the walk do not depend on the conversion mode, no walk reaches the step cap,
    and the walk's id and t are the brute force's bit for bit on the 8192 incoherent rays and the hostile-ray families that are in general position to a
    scene (a - h; i, j and l have no brute force to be held to: tests/test_hostile_rays_cpu.py holds them to float64 and to the contract).  Rays that lie in
    the plane of a flat triangle are left out by S.in_plane_mask: at most 1 % of either batch."""
    tris, G, rays, fam = _flat(name, compress)
    rc, msg = G.check(tris, 1)
    assert rc == 0, msg
    O.walk_capped()
    hits, stats, steps = G.traverse(tris, rays, want_steps=True)
    with O.walk_mode(O.DEVICE_F2I):
        G2 = O.Grid.full(tris, compress=compress)
        hits2, stats2, steps2 = G2.traverse(tris, rays, want_steps=True)
    assert O.walk_capped() == (0, -1)
    assert same_grid(G, G2)
    assert (words(hits) == words(hits2)).all() and stats == stats2 and (steps == steps2).all()
    bf = O.brute_force(tris, rays, nthreads=8)
    mask = S.in_plane_mask(tris, rays)
    base = fam == "0"
    print(name, "masked:", int(mask[base].sum()), "of", int(base.sum()), "incoherent rays,", int(mask[~base].sum()), "of", int((~base).sum()), "catalogue rays; hits:",
          int((bf["id"][base] >= 0).sum()))
    assert mask[base].mean() <= S.MASK_CAP and mask[~base].mean() <= S.MASK_CAP
    compared = np.isin(fam, list("0abcdefgh")) & ~mask
    bad = compared & ((hits["id"] != bf["id"]) | (H.bits(hits["t"]) != H.bits(bf["t"])))
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:5], fam[bad][:5], hits[bad][:3], bf[bad][:3])
    j = fam == "j"
    assert (words(hits[j]) == H.contract_records(rays[j])).all()
    if name not in ("point", "line"):                      # (zero-area triangles are hit by no ray)
        assert (bf["id"][base] >= 0).sum() > 50


NONFINITE = S.nonfinite_scenes()


@pytest.mark.parametrize("case", NONFINITE, ids=[c[0] for c in NONFINITE])
def test_oracle_refuses_nonfinite_scenes(case):
    """EINVAL for an inadmissible triangle wherever it stands, ERANGE (box) for finite triangles whose extent overflows; the grid is left untouched, and the
    clean soup builds right after"""
    name, tris, answer, row = case
    rc, G = orc_build(tris)
    assert rc == (ORC_EINVAL if answer == S.EINVAL else ORC_ERANGE_BOX)
    assert not G.g.entries and not G.g.cells and not G.g.ref_ids and G.g.num_cells == 0
    if row is not None:
        bad = [i for i in range(tris.shape[0]) if not O.lib().orc_tri_admissible(tris[i:i + 1].ctypes.data_as(C.c_void_p))]
        assert bad == [row]
    rc, G = orc_build(S.clean_soup())
    assert rc == 0 and G.num_refs > 0


def test_derived_vertices_make_a_triangle_inadmissible():
    """twelve finite floats whose v0 - e1 or v0 + e2 overflows"""
    t = S.clean_soup()[:8].copy()
    t[2, 0] = np.float32(3e38); t[2, 4] = np.float32(-3e38)
    assert np.isfinite(t).all() and orc_build(t)[0] == ORC_EINVAL
    t = S.clean_soup()[:8].copy()
    t[5, 2] = np.float32(-3e38); t[5, 10] = np.float32(-3e38)
    assert np.isfinite(t).all() and orc_build(t)[0] == ORC_EINVAL
    assert orc_build(t[:0])[0] == ORC_EINVAL


@pytest.mark.parametrize("band,tris", S.size_scenes(), ids=[b for b, _ in S.size_scenes()])
def test_oracle_refuses_reference_totals_beyond_the_limit(band, tris):
    total = S.top_reference_total(tris)
    print("band", band, "total", total, "= 2^%.2f" % np.log2(total), "mod 2^32:", total % 2 ** 32)
    assert S.BANDS[band](total)
    rc, G = orc_build(tris)
    assert rc == ORC_ERANGE and not G.g.entries


@pytest.mark.parametrize("snd", [1e22, 1e30])
def test_oracle_refuses_a_second_level_of_24_levels(snd):
    """a second-level density at which Cleary's formula asks for 2^23 cells or more along an axis of a top-level cell (1e22), and one at which the product
    leaves int's range and the total function answers INT_MAX (1e30): 24 levels or more either way"""
    rc, G = orc_build(S.clean_soup(), snd=snd)
    assert rc == ORC_ERANGE_LEVELS and not G.g.entries


def test_oracle_build_under_sanitizers(tmp_path):
    """tests/cpp/hostile_scenes_host.cpp with oracle/hagrid_oracle.c as a stand-alone program with -fsanitize=address,undefined,float-cast-overflow (leak check
    included).  First the total functions: compute_grid_dims, grid_dims_defined, widen_scene_box, compute_range and tri_admissible of the headers (what the
    device compiles) against the oracle's restatements, the documented values where the formulas are undefined and equal results on boxes with zero, denormal,
    huge, infinite and NaN extents.  Then orc_build_grid, merge, flatten, expand, the grid check and compress over every catalogue: no report, the expected
    answers."""
    exe = str(tmp_path / "hostile_scenes_host")
    san = ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off"]
    obj = str(tmp_path / "hagrid_oracle.o")
    subprocess.run(["gcc", "-std=gnu11", *san, "-c", os.path.join(ROOT, "oracle", "hagrid_oracle.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++11", *san, "-Wall", "-DHOST=", "-DDEVICE=", "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "hostile_scenes_host.cpp"), obj, "-o", exe, "-lm", "-lpthread"], check=True)
    scenes = [(n, t, 0) for n, t in FLAT.items()]
    scenes += [(n, t, ORC_EINVAL if a == S.EINVAL else ORC_ERANGE_BOX) for n, t, a, _ in NONFINITE]
    scenes += [("size-" + b, t, ORC_ERANGE) for b, t in S.size_scenes()]
    scenes.append(("clean", S.clean_soup(), 0))
    lines = []
    for i, (n, t, want) in enumerate(scenes):
        path = str(tmp_path / f"s{i}.bin")
        np.ascontiguousarray(t, np.float32).tofile(path)
        lines.append(f"{path} {t.shape[0]} {want}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(tmp_path / "list.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "total functions: 20000 inputs compared" in r.stdout and r.stdout.count("ok ") == len(scenes)
