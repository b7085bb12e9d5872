"""What test_fallbacks_cpu.py and test_fallbacks_gpu.py share: the scenes that put a pass on a branch it takes only when a count crosses a constant (more than
2048 large primitives, more tasks than resident wavefronts, expansions whose cells still grow), and the reach conditions that numpy can state about them."""
import numpy as np

from hagrid_amd import scene

COOP_CELLS = 64             # build.hip kCoopCells: a primitive whose box covers this many top-level cells is a large one
BIG_BLOCKS = 2048           # build.hip: the workgroups the large primitives get in count_top_refs / emit_top_refs
NEEDLE_COUNTS = (2048, 2049, 3000)


def needles(m: int, seed: int = 4242) -> np.ndarray:
    """m triangles with one vertex in [0, 0.15]^3, one in [0.85, 1]^3 and the third at their midpoint +- 0.005: a box that spans the scene, a surface that
    meets few cells"""
    u = scene.uniform01(seed, np.arange(m, dtype=np.uint64)[:, None] * np.uint64(9) + np.arange(9, dtype=np.uint64)[None, :])
    a = u[:, 0:3] * np.float32(0.15)
    b = np.float32(0.85) + u[:, 3:6] * np.float32(0.15)
    c = (a + b) * np.float32(0.5) + (np.float32(2.0) * u[:, 6:9] - np.float32(1.0)) * np.float32(0.005)
    return scene.tris_from_vertices(a, b, c)


def needle_scene(m: int) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([scene.make_soup(2000, seed=7), needles(m)]), dtype=np.float32)


def top_cells_covered(tris: np.ndarray, dims, bbox_min, bbox_max) -> np.ndarray:
    """per triangle the number of top-level cells its box covers, in float64 (the construction's compute_range: floor of the box's corners in cell units,
    clamped to the grid)"""
    lo = np.asarray(bbox_min, np.float64); ext = np.asarray(bbox_max, np.float64) - lo
    d = np.asarray(dims, np.float64)
    v = scene.tri_vertices(tris).astype(np.float64).reshape(-1, 3, 3)
    first = np.clip(np.floor((v.min(axis=1) - lo) / ext * d), 0, d - 1)
    last = np.clip(np.floor((v.max(axis=1) - lo) / ext * d), 0, d - 1)
    return np.prod(last - first + 1, axis=1).astype(np.int64)


def large_primitives(tris: np.ndarray, dims, bbox_min, bbox_max) -> int:
    return int((top_cells_covered(tris, dims, bbox_min, bbox_max) >= COOP_CELLS).sum())


# ---- the distance lattice whose every box is the whole lattice ---------------------------------------------------------------------------

def whole_lattice_case(n=(64, 64, 32)):
    """(tris, origin, size, n, band): 200 triangles, a lattice over the scene box, a band wider than the scene -- every triangle's voxel box is the whole lattice"""
    tris = scene.make_soup(200, seed=21)
    lo, hi = scene.tris_bbox(tris)
    size = ((hi - lo) / np.float32(n)).astype(np.float32)
    return tris, lo, size, tuple(n), 4.0


# ---- expansions whose cells still grow ---------------------------------------------------------------------------------------------------

EXPAND_SCENES = {           # name: (triangles, top density, second density, alpha)
    "soup4000": (lambda: scene.make_soup(4000), 0.12, 2.4, 0.995),
    "soup1500_fine": (lambda: scene.make_soup(1500), 1.5, 12.0, 0.0),
    "soup333_fine": (lambda: scene.make_soup(333), 1.5, 12.0, 0.0),
    "clustered": (lambda: scene.make_clustered(2000, 2, 3000), 0.12, 2.4, 0.995),
}


def expand_scene(name: str):
    make, td, sd, alpha = EXPAND_SCENES[name]
    return np.ascontiguousarray(make(), dtype=np.float32), td, sd, alpha


def oracle_before_expansion(name: str):
    """(tris, the oracle's grid built, merged and flattened)"""
    from oracle import oracle as O
    tris, td, sd, alpha = expand_scene(name)
    return tris, O.Grid.build(tris, td, sd).merge(alpha).flatten()


def oracle_expansions(name: str, iters, subset_only: bool = True) -> dict:
    """{k: the cells of the oracle's expand(k) from the fresh grid} for every k of `iters` (the grid is built once: an expansion changes the cells alone, and
    they are put back before the next one)"""
    tris, G = oracle_before_expansion(name)
    fresh = G.cells.copy()
    out = {}
    for k in sorted(set(iters)):
        G.cells[:] = fresh
        out[k] = G.expand(tris, k, subset_only=subset_only).cells.copy()
    return out


def cells_differ(a: np.ndarray, b: np.ndarray) -> int:
    return int(((a["min"] != b["min"]).any(axis=1) | (a["max"] != b["max"]).any(axis=1)).sum())
