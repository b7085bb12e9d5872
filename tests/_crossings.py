"""What the crossing tests and the fixture generator (tests/golden/make_golden_crossings.py) share: the scenes, rays and points of the fixture, the
records made from per-pair results, and the host program tests/cpp/crossings_host.cpp (the header's brute force and the header's walk) as callables."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _host
import _multi_hit as M
from _host import ROOT, INC, oracle_grid, oracle_grid_arrays                # names the tests use

FIXTURE = os.path.join(ROOT, "tests", "golden", "crossings.npz")
SCENES = ("soup", "mesh", "solids")
DETAIL = 0.05
PAGES = (1, 2, 3, 4, 8)             # page capacities of the host walk; the kernel's is 8
NUM_POINTS = 2048
LATTICE = (16, 16, 16)
BAND = (0.7, 1.15)                  # of a solid's (tube) radius: no fixture point lies that close to an analytic surface (the tessellation lies in the band)


def make_tris(name: str) -> np.ndarray:
    if name == "solids":
        return scene.make_closed_solids(DETAIL)[0]
    return M.make_tris(name)


def base_rays(name: str, tris: np.ndarray) -> np.ndarray:
    """soup, mesh: exactly the rays of multi_hit.npz; solids: 48 x 48 primary rays plus 1792 incoherent ones, every ray with its full window"""
    if name != "solids":
        return M.fixture_rays(tris)
    lo, hi = scene.tris_bbox(tris)
    return np.concatenate([scene.make_rays_primary(lo, hi, 48, 48), scene.make_rays_incoherent(lo, hi, 1792, 3)]).astype(np.float32)


def aimed_rays(tris: np.ndarray, count: int, seed: int) -> np.ndarray:
    """rays through the whole scene that start outside it: from a point on a sphere around the box towards a surface sample -- they cross many surfaces"""
    lo, hi = scene.tris_bbox(tris)
    centre = ((lo + hi) * np.float32(0.5)).astype(np.float32)
    target, _ = scene.make_points_surface(tris, count, seed)
    g = scene.make_gaussian3(seed ^ 0x61696d, count)
    g = g / np.maximum(np.sqrt((g * g).sum(axis=1, keepdims=True)), np.float32(1e-6))
    org = (centre + g * scene.bbox_diagonal(lo, hi)).astype(np.float32)
    rays = np.zeros((count, 8), dtype=np.float32)
    rays[:, 0:3] = org; rays[:, 4:7] = (target - org).astype(np.float32); rays[:, 7] = np.float32(np.inf)
    return rays


def paging_counts(page: int):
    """the counts every scene must show for the paging of capacity `page` to be exercised: 0, 1, P, P + 1, 2P and something beyond 2P"""
    return (0, 1, page, page + 1, 2 * page)


# Which page capacities each scene's rays cover in full.  A straight line crosses a torus at most four times and a sphere twice; through the ten closed
# solids no line was found with more than ten crossings (24 x 24 lines between the ring circles and centres of every pair of solids: at most eight;
# 16384 aimed rays: at most ten), so 2P and "more than 2P" for P = 8 do not exist there.  The solids scene covers P = 4 in full; the host walk runs it
# with capacities 1 .. 4 as well.
COVERED_PAGES = {"soup": (4, 8), "mesh": (4, 8), "solids": (4,)}


def has_paging_coverage(counts: np.ndarray, pages=(4, 8)) -> bool:
    c = set(int(v) for v in counts)
    return all(all(v in c for v in paging_counts(p)) and max(c) > 2 * p for p in pages)


def records_from_pairs(rays: np.ndarray, ray_idx, tri_idx, t, entering) -> np.ndarray:
    """the records (scene.HIT_DTYPE) of the crossings listed as parallel arrays (ray, triangle, t, entering): sort by (t, id), count, first t, the sequential
    float32 sum over pairs, winding -- the definition of include/hagrid/crossings.h written independently of scene.ray_crossings"""
    n = rays.shape[0]
    out = np.zeros(n, dtype=scene.HIT_DTYPE)
    out["t"] = rays[:, 7]
    order = np.lexsort((tri_idx, t, ray_idx))
    ray_idx, t, entering = np.asarray(ray_idx)[order], np.asarray(t, np.float32)[order], np.asarray(entering)[order]
    winding = np.zeros(n, dtype=np.int32)
    start = np.searchsorted(ray_idx, np.arange(n)); stop = np.searchsorted(ray_idx, np.arange(n), side="right")
    for i in np.flatnonzero(stop > start):
        tt = t[start[i]:stop[i]]
        acc = np.float32(0.0)
        for p in range(tt.size // 2):
            acc = np.float32(acc + np.float32(tt[2 * p + 1] - tt[2 * p]))
        out["id"][i] = tt.size; out["t"][i] = tt[0]; out["u"][i] = acc
        e = entering[start[i]:stop[i]]
        winding[i] = int((~e).sum()) - int(e.sum())
    out["v"] = winding.view(np.float32)
    return out


def make_points(tris: np.ndarray, solids: list) -> tuple[np.ndarray, np.ndarray]:
    """(points (NUM_POINTS, 4) float32 with reach +inf, labels (NUM_POINTS,) int32): make_points_uniform and make_points_near_surface points, none closer to the analytic surface
    of ANY solid than BAND allows; the first NUM_POINTS survivors.  label = the number of solids that contain the point is odd."""
    lo, hi = scene.tris_bbox(tris)
    # three families, taken in turn: uniform over the scene, near the surface, and -- the solids fill a few per cent of the scene's box -- uniform over
    # the box of each solid's own triangles, so that at least a quarter of the points lie inside
    per = 1024
    fam = [scene.make_points_uniform(lo, hi, per, 11, enlarge=0.05), scene.make_points_near_surface(tris, lo, hi, per, 12, sigma=0.01)]
    for k, s in enumerate(solids):
        first, count = s["faces"]
        slo, shi = scene.tris_bbox(tris[first:first + count])
        fam.append(scene.make_points_uniform(slo, shi, per, 13 + k, enlarge=0.0))
    cand = np.stack(fam, axis=1).reshape(-1, 3)
    keep = np.ones(cand.shape[0], dtype=bool)
    containing = np.zeros(cand.shape[0], dtype=np.int64)
    for s in solids:
        r = s["radii"][-1]
        rel = (scene.solid_distance(s, cand) + r) / r            # distance to the centre (line) in units of the (tube) radius: 1 on the surface
        keep &= ~((rel >= BAND[0]) & (rel <= BAND[1]))
        containing += rel < 1.0
    idx = np.flatnonzero(keep)[:NUM_POINTS]
    assert idx.size == NUM_POINTS, "not enough points survive the band"
    pts = np.zeros((NUM_POINTS, 4), dtype=np.float32)
    pts[:, 0:3] = cand[idx]; pts[:, 3] = np.float32(np.inf)
    return pts, (containing[idx] & 1).astype(np.int32)


def lattice_of(tris: np.ndarray):
    """(origin, size, n): LATTICE over the bounding box of the triangles"""
    lo, hi = scene.tris_bbox(tris)
    n = np.array(LATTICE, np.int32)
    return lo.astype(np.float32), ((hi - lo) / n.astype(np.float32)).astype(np.float32), n


def checksum(a: np.ndarray) -> int:
    w = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64).reshape(-1)
    return int(((w * (np.arange(w.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64)) & np.uint64(0xFFFFFFFFFFFFFFFF))


def rec_bits(records) -> np.ndarray:
    """(n, 4) uint32 of HIT_DTYPE records"""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 4)


# ---- tests/cpp/crossings_host.cpp ------------------------------------------------------------------------------------------------

def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("crossings_host", directory, sanitize)


def _query_params(form: int, n: int, dirs, winding: bool, lattice) -> tuple[bytes, int]:
    d = scene.CROSSING_DIRS.copy().reshape(-1)
    m = 1 if form == 0 else 3
    if dirs is not None:
        dd = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        m = dd.shape[0]; d[:3 * m] = dd.reshape(-1)
    origin, size, ln = lattice if lattice is not None else (np.zeros(3, np.float32), np.ones(3, np.float32), np.ones(3, np.int32))
    return struct.pack("<iiii9f3f3f3i", form, n, m, 1 if winding else 0, *[float(v) for v in d], *[float(v) for v in origin], *[float(v) for v in size],
                       *[int(v) for v in ln]), m


def host_query(exe: str, directory, tris: np.ndarray, grid: dict | None = None, page: int = 8, rays=None, points=None, lattice=None, dirs=None,
               winding: bool = False, paged: bool = False) -> dict:
    """The host program over rays (n, 8), points (n, 4) or a lattice (origin, size, n).  grid None: the brute force (paged: the header's crossings_brute_force; else the same definition by a sort); else the header's walk over
    grid arrays (keys entries, ref_ids, cells | small_cells, bbox_min, bbox_max, dims, shift) with page capacity `page`.  Returns "records" (n, m)
    HIT_DTYPE, "inside" (n,) int32, "totals" int64[4] (items, cells, tests, flushes) and "excess" (flushes beyond ceil(count / page) + 1, the largest)."""
    d = str(directory)
    form = 0 if rays is not None else (1 if points is not None else 2)
    items = rays if form == 0 else (points if form == 1 else np.zeros(0, np.float32))
    n = int(np.prod(lattice[2])) if form == 2 else int(np.ascontiguousarray(items).view(np.float32).size // (8 if form == 0 else 4))
    params, m = _query_params(form, n, dirs, winding, lattice)
    par = os.path.join(d, "cx_params.bin")
    args = [exe, ("paged" if paged else "brute") if grid is None else "walk", par]
    if grid is not None:
        params += _host.grid_header(grid) + struct.pack("<i", int(page))
        args += _host.grid_files(d, grid, "cx_")
    with open(par, "wb") as f:
        f.write(params)
    out = os.path.join(d, "cx_out.bin")
    subprocess.run(args + [_host.put(d, "cx_tris", np.ascontiguousarray(tris, dtype=np.float32)), _host.put(d, "cx_items", np.ascontiguousarray(items).view(np.float32)), out],
                   check=True, timeout=900)
    raw = np.fromfile(out, dtype=np.uint8)
    nrec = n * m * 16
    tail = raw[nrec + 4 * n:].view(np.int64)
    return {"records": raw[:nrec].view(scene.HIT_DTYPE).reshape(n, m), "inside": raw[nrec:nrec + 4 * n].view(np.int32), "totals": tail[:4].copy(),
            "excess": int(tail[4])}


def empty_records(rays: np.ndarray) -> np.ndarray:
    """what a ray that takes no cell step gets: count 0, t = the bits of its tmax, length +0, winding 0; (n, 4) uint32"""
    rec = np.zeros((rays.shape[0], 4), np.uint32)
    rec[:, 1] = np.ascontiguousarray(rays[:, 7], dtype=np.float32).view(np.uint32)
    return rec


def assert_records_equal(got, want, what: str):
    g, w = rec_bits(got), rec_bits(want)
    assert g.shape == w.shape, f"{what}: {g.shape} against {w.shape}"
    bad = (g != w).any(axis=1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} records differ, first at {np.flatnonzero(bad)[:5]}: got {g[bad][:2]}, want {w[bad][:2]}"


def assert_hostile_records(got, want, family, what: str):
    """The device's or the host walk's records of the catalogue of tests/_hostile_rays.py against the brute force's, by the catalogue's own contract
    (tests/test_hostile_rays_cpu.py): every family bit for bit, except
      (i) origins 1e3 .. 1e6 diagonals away and (l) directions whose det underflows for every triangle: float32 decides nothing there, the brute force accepts
          triangles nowhere near the ray ("no brute force to speak of") -- such rays are held to termination, the flush bound and device = host walk;
      (k) rays through vertices, along edges and inside triangle planes: the brute force accepts a neighbour by the -1e-9 slack at a point in a cell that does
          not list it; at most AMBIGUOUS_CAP of the family may differ, as for the nearest hit."""
    import _hostile_rays as H
    bad = (rec_bits(got) != rec_bits(want)).any(axis=1)
    strict = ~np.isin(family, ["i", "k", "l"])
    assert not (bad & strict).any(), f"{what}: {(bad & strict).sum()} rays differ, families {sorted(set(family[bad & strict]))}, first at {np.flatnonzero(bad & strict)[:5]}"
    k = family == "k"
    if k.any():
        assert (bad & k).sum() <= H.AMBIGUOUS_CAP * k.sum(), f"{what}: {(bad & k).sum()} of {k.sum()} rays of family (k) differ"
    assert strict.sum() > 3000
