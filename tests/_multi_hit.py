"""What the multi-hit tests and the fixture generator (tests/golden/make_golden_multi_hit.py) share: the scenes and rays of the fixture, the
per-triangle brute force that states the semantics (every triangle alone through the oracle's intersect_prim_ray, the ray's own window,
then a sort by (t, id)), and the host walk tests/cpp/multi_hit_host.cpp as a callable."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _host
from _host import ROOT, INC, SANITIZE, bits, oracle_grid_arrays               # names the tests use

FIXTURE = os.path.join(ROOT, "tests", "golden", "multi_hit.npz")
KMAX = 8
SCENES = ("soup", "mesh")


def make_tris(name: str) -> np.ndarray:
    return scene.make_soup(20000, seed=7) if name == "soup" else scene.make_stadium(0.05)


def mixed_rays(tris: np.ndarray, width: int, height: int, num_incoherent: int) -> np.ndarray:
    """width x height primary rays, then incoherent rays (seed 3); every fifth ray gets a finite window: tmin 0.05, tmax 0.6 |bbox diagonal|"""
    lo, hi = scene.tris_bbox(tris)
    rays = np.concatenate([scene.make_rays_primary(lo, hi, width, height), scene.make_rays_incoherent(lo, hi, num_incoherent, 3)]).astype(np.float32)
    ext = hi - lo
    diag = np.float32(np.sqrt(np.float32(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2])))
    rays[::5, 3] = np.float32(0.05)
    rays[::5, 7] = np.float32(0.6) * diag
    return rays


def fixture_rays(tris: np.ndarray) -> np.ndarray:
    return mixed_rays(tris, 48, 48, 1792)


def lists_by_brute_force(tris: np.ndarray, rays: np.ndarray, use_ref: bool = False, k: int = KMAX):
    """(ids [n, k], t [n, k]): for every triangle j alone, oracle.brute_force(tris[j:j+1], rays) says whether ray i intersects it and at
    which t (use_ref: through the reference's own headers); per ray the k smallest by (t, id); unused slots id -1, t = the ray's tmax."""
    from oracle import oracle as O
    n = rays.shape[0]
    ray_idx, tri_idx, ts = [], [], []
    for j in range(tris.shape[0]):
        h = O.brute_force(tris[j:j + 1], rays, use_ref=use_ref)
        on = np.flatnonzero(h["id"] >= 0)
        if on.size:
            ray_idx.append(on); tri_idx.append(np.full(on.size, j, dtype=np.int32)); ts.append(h["t"][on])
    ids = np.full((n, k), -1, dtype=np.int32)
    t = np.repeat(rays[:, 7:8], k, axis=1).astype(np.float32)
    if ray_idx:
        r = np.concatenate(ray_idx); j = np.concatenate(tri_idx); tt = np.concatenate(ts)
        order = np.lexsort((j, tt, r))             # by ray, then t, then id
        r, j, tt = r[order], j[order], tt[order]
        first = np.searchsorted(r, np.arange(n))
        slot = np.arange(r.size) - first[r]
        keep = slot < k
        ids[r[keep], slot[keep]] = j[keep]
        t[r[keep], slot[keep]] = tt[keep]
    return ids, t


def hit_histogram(ids: np.ndarray) -> list:
    return np.bincount((ids >= 0).sum(axis=1), minlength=ids.shape[1] + 1).tolist()


def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("multi_hit_host", directory, sanitize)


def host_walk(exe: str, directory, grid: dict, tris: np.ndarray, rays: np.ndarray, k: int) -> np.ndarray:
    """The host walk over grid arrays (keys entries, ref_ids, cells | small_cells, bbox_min, bbox_max, dims, shift: what api.Grid.download
    returns); the hits as an (n, k) HIT_DTYPE array."""
    d = str(directory)
    n = rays.shape[0]
    par = os.path.join(d, "params.bin")
    with open(par, "wb") as f:
        f.write(_host.grid_header(grid) + struct.pack("<ii", k, n))
    out = os.path.join(d, "out.bin")
    subprocess.run([exe, "walk", par, *_host.grid_files(d, grid), _host.put(d, "tris", np.ascontiguousarray(tris, dtype=np.float32)),
                    _host.put(d, "rays", np.ascontiguousarray(rays, dtype=np.float32)), out], check=True, timeout=600)
    return np.fromfile(out, dtype=scene.HIT_DTYPE).reshape(n, k)
