"""What the distance-lattice tests (hagrid_distance_lattice: test_distance_lattice_cpu.py, test_distance_lattice_gpu.py) and the fixture generator
(tests/golden/make_golden_distance_lattice.py) share: the cases of the fixture (scenes and lattices of _fill_lattice, two bands each), the fixture's keys, the
numpy count of pairs within the band, and the host program tests/cpp/distance_host.cpp (the definition and the header's scatter) as a callable."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _fill_lattice as F
import _host

FIXTURE = os.path.join(_host.ROOT, "tests", "golden", "distance_lattice.npz")
KEYS = ("boxes_a", "boxes_b", "boxes_c", "soup_a", "mesh_a", "solids_a", "solids_brick")
BAND_FACTORS = (1.5, 3.0)           # bands in units of the largest voxel edge
TASK_VOXELS = 2048                  # hagrid::distance::kTaskVoxels


def band_of(size, factor) -> np.float32:
    return np.float32(factor) * np.asarray(size, np.float32).max()


def all_cases():
    """(scene name, key, origin, size, n) of every lattice of the fixture"""
    return [c for c in F.all_cases() if c[1] in KEYS]


_tris = {}


def tris_of(name: str) -> np.ndarray:
    if name not in _tris:
        _tris[name] = F.make_tris(name)
    return _tris[name]


def case(key: str):
    """(tris, origin, size, n) of one lattice of _fill_lattice by its key (the fixture's and the others: boxes_one, boxes_flat)"""
    name = key.rsplit("_", 1)[0]
    tris = tris_of(name)
    for k, origin, size, n in F.lattices(name, tris):
        if k == key:
            return tris, origin, size, n
    raise KeyError(key)


def pairs_within(tris: np.ndarray, origin, size, n, band, chunk_pairs: int = 1 << 21) -> int:
    """how many (triangle with a surface, voxel centre) pairs have d2 <= band * band: counter 2 of hagrid_distance_lattice"""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    P = np.ascontiguousarray(scene.lattice_centres(origin, size, n)["p"])
    cols = [T[None, :, i] for i in range(12)]
    r2 = np.float32(band) * np.float32(band)
    m = max(1, chunk_pairs // max(T.shape[0], 1))
    total = 0
    with np.errstate(all="ignore"):
        for o in range(0, P.shape[0], m):
            p = P[o:o + m]
            valid, d2 = scene._point_tri((p[:, 0:1], p[:, 1:2], p[:, 2:3]), cols, False)
            total += int((valid & (d2 <= r2)).sum())
    return total


def fixture_records(fx, key: str, b: int) -> np.ndarray:
    """the answers of lattice `key` with band BAND_FACTORS[b] as CLOSEST_DTYPE records"""
    ids = fx[key + "_id"][b]
    r = np.zeros(ids.size, dtype=scene.CLOSEST_DTYPE)
    r["id"] = ids; r["d2"] = fx[key + "_d2"][b]; r["q"] = fx[key + "_q"][b]
    r["feature"] = fx[key + "_feature"][b]; r["side"] = fx[key + "_side"][b].astype(np.float32)
    return r


def assert_records_equal(got: np.ndarray, want: np.ndarray, what: str):
    """CLOSEST_DTYPE records, all 32 bytes, no voxel excepted"""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 8); w = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 8)
    assert g.shape == w.shape, f"{what}: {g.shape} against {w.shape}"
    bad = (g != w).any(axis=1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} voxels differ, first at {np.flatnonzero(bad)[:5]}: got {got[bad][:2]}, want {want[bad][:2]}"


# ---- tests/cpp/distance_host.cpp ------------------------------------------------------------------------------------------------------

def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("distance_host", directory, sanitize)


def host_distance(exe: str, directory, tris: np.ndarray, origin, size, n, band, op: str = "scatter", task_voxels: int = TASK_VOXELS, reverse: bool = False,
                  grid_box=None):
    """The host program over a lattice.  op "brute": the definition; "scatter": sizes -> sums -> tasks -> splat -> finish with `task_voxels` per task, the tasks
    taken last first with `reverse`.  Returns (CLOSEST_DTYPE records, int64[4]: triangles with a voxel box, tasks, pairs within the band, voxels with an answer)."""
    d = str(directory)
    lo, hi = grid_box if grid_box is not None else scene.tris_bbox(tris)
    par = os.path.join(d, "dl_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<3f3f3if3f3fii", *[float(v) for v in origin], *[float(v) for v in size], *[int(v) for v in n], float(band), *[float(v) for v in lo],
                            *[float(v) for v in hi], int(task_voxels), 1 if reverse else 0))
    out = os.path.join(d, "dl_out.bin")
    subprocess.run([exe, op, par, _host.put(d, "dl_tris", np.ascontiguousarray(tris, dtype=np.float32)), out], check=True, timeout=900)
    raw = np.fromfile(out, dtype=np.uint8)
    voxels = int(np.prod([int(v) for v in n]))
    return raw[:32 * voxels].view(scene.CLOSEST_DTYPE).copy(), raw[32 * voxels:].view(np.int64)[:4].copy()
