"""What the hostile-scene tests (tests/test_hostile_scenes_cpu.py, tests/test_hostile_scenes_gpu.py) share: seeded catalogues of scenes a caller can hand
to hagrid_build_grid and the project's own generators never produce ("Admissible scenes") -- flat scenes, whose box has no
volume; scenes with non-finite triangles, which are refused; thin slabs, whose reference totals leave 32 bits -- the rays that go with a flat scene,
and the 64-bit reference total of a scene restated with numpy.  Every fixture is packed by scene.tris_from_vertices."""
import numpy as np

from hagrid_amd import scene

import _hostile_rays as H

F32 = np.float32
SEED = 0x666C6174                   # "flat"
TOP_DENSITY, SND_DENSITY = 0.12, 2.4          # the default construction parameters
WIDEN_FRACTION = F32(2.0 ** -10)    # include/hagrid/grid.h kWidenFraction
WIDEN_MIN_SCALE = F32(2.0 ** -20)   # include/hagrid/grid.h kWidenMinScale
# (dims, shift, cells, references) of every flat fixture after orc_build_grid with the default densities, as DESIGN.md section 2 records them
RECORDED = {"one_triangle": ((4, 2, 4), 3, 1425, 551),
            "quad": ((10, 4, 2), 4, 23880, 10455),
            "plane_z025": ((30, 28, 2), 3, 29561, 6036),
            "plane_z0": ((30, 28, 2), 3, 29561, 6036),
            "plane_x_3000": ((2, 64, 62), 4, 95135, 18133),
            "line": ((2, 184, 2), 5, 36457, 152807),
            "point": ((2, 2, 2), 2, 22, 37),
            "plane_thin_1e-30": ((30, 28, 2), 3, 29561, 6036),
            "plane_one_ulp": ((30, 28, 2), 3, 29561, 6036)}
MASK_CAP = 0.01                     # the largest share of a batch that may lie in a flat scene's own plane


def _u(seed, count, width):
    return scene._uniform_rows(SEED + seed, count, width)


def _lattice(n, seed, x0, y0, side):
    """n triangles in the square (x0, y0) + [0, side)^2, one per square of a g x g lattice, g = ceil(sqrt(n)): three random points of the inner 90 % of its
    square each.  No two triangles overlap or touch: a ray that crosses the plane meets one triangle at most, so the nearest hit is no tie between
    coplanar triangles (which the walk and the brute force break differently: DESIGN.md section 6, D6)."""
    g = int(np.ceil(np.sqrt(n)))
    u = _u(seed, n, 6)
    i = np.arange(n)
    corner = np.stack([i % g, i // g], axis=1).astype(F32)
    cell = F32(side) / F32(g)
    p = np.empty((3, n, 2), F32)
    for k in range(3):
        p[k] = (np.array([x0, y0], F32) + (corner + F32(0.05) + F32(0.9) * u[:, 2 * k:2 * k + 2]) * cell).astype(F32)
    return p


def _planar(n, seed, axis, value, clusters=0, per_cluster=0):
    """n lattice triangles in the unit square of the plane `axis` = value, then `clusters` groups of `per_cluster` lattice triangles, each group in a square of
    side 0.002 beside the unit square: a group is smaller than the finest cell the construction gives it, so its triangles share reference lists"""
    parts = [_lattice(n, seed, 0.0, 0.0, 1.0)]
    for c in range(clusters):
        parts.append(_lattice(per_cluster, seed + 100 + c, 1.05, c / max(clusters, 1), 0.002))
    p = np.concatenate(parts, axis=1)
    v = np.full((3, p.shape[1], 3), F32(value), F32)
    others = [a for a in range(3) if a != axis]
    for k in range(3):
        v[k][:, others[0]] = p[k][:, 0]; v[k][:, others[1]] = p[k][:, 1]
    return v


def _pack(v):
    return scene.tris_from_vertices(v[0], v[1], v[2])


def flat_scenes() -> dict:
    """name -> (n, 12) float32.  Every scene's box has an extent that is zero, or so small that density * n / volume or a product extent * ratio leaves
    float's or int's range: Cleary's formula is undefined for it and the box is widened (grid.h widen_scene_box)."""
    S = {}
    S["one_triangle"] = _pack(np.array([[[0.25, 0.5, 0.75]], [[1.0, 0.5, 0.75]], [[0.25, 0.5, 1.5]]], F32))            # in the plane y = 0.5
    q = np.array([[0, 0, 2], [3, 0, 2], [3, 1, 2], [0, 1, 2]], F32)
    S["quad"] = scene.tris_from_vertices(q[[0, 0]], q[[1, 2]], q[[2, 3]])
    S["plane_z025"] = _pack(_planar(200, 1, 2, 0.25))
    S["plane_z0"] = _pack(_planar(200, 1, 2, 0.0))
    # long lists: 25 groups of 40 triangles in one cell each.  The scene is 1024 units wide: the reference's ray test accepts u, v, w >= -1e-9 whatever the
    # size of the triangle, so in a unit scene a group's triangles (1e-4 wide) would be "hit" by rays that pass them at twenty times their size
    S["plane_x_3000"] = _pack(_planar(2000, 2, 0, -1.5, clusters=25, per_cluster=40) * F32(1024))
    t = _u(3, 50, 3)
    line = lambda s: np.stack([F32(0.5) + F32(0) * s, s, F32(-0.25) + F32(0) * s], axis=1).astype(F32)
    S["line"] = scene.tris_from_vertices(line(t[:, 0]), line(t[:, 1]), line(t[:, 2]))         # collinear vertices on a line along y: two zero extents
    pt = np.tile(np.array([[0.3, -0.7, 1.1]], F32), (37, 1))
    S["point"] = scene.tris_from_vertices(pt, pt, pt)
    v = _planar(200, 1, 2, 0.0)
    v[1][::2, 2] = F32(1e-30)                                                       # every other triangle's second vertex: a z extent of 1e-30
    S["plane_thin_1e-30"] = _pack(v)
    v = _planar(200, 1, 2, 0.0)
    v[:, 17, 2] = np.nextafter(F32(0), F32(1))                                      # one triangle lifted by one ulp of the plane's coordinate
    S["plane_one_ulp"] = _pack(v)
    return S


def flat_coordinates(tris):
    """per axis, the coordinates at which the scene holds an axis-aligned flat triangle (all three vertices share the coordinate)"""
    v0 = tris[:, 0:3]; v1 = v0 - tris[:, 4:7]; v2 = v0 + tris[:, 8:11]
    return [np.unique(v0[(v0[:, a] == v1[:, a]) & (v0[:, a] == v2[:, a]), a]) for a in range(3)]


def in_plane_mask(tris, rays) -> np.ndarray:
    """The stated mask: rays that lie IN the plane of an axis-aligned flat triangle of the scene -- the direction component of that axis is zero and the
    origin's coordinate is the plane's.  Every |det| such a ray meets there is zero; the reference's arithmetic decides nothing for it."""
    m = np.zeros(rays.shape[0], bool)
    for a, c in enumerate(flat_coordinates(tris)):
        m |= (rays[:, 4 + a] == 0) & np.isin(rays[:, a], c)
    return m


def scene_rays(tris, G):
    """(rays, family): 8192 incoherent rays from the grid's box enlarged by a quarter of its largest extent, then the hostile-ray catalogue of the grid
    (family letters of tests/_hostile_rays.py; the incoherent rays are family "0")"""
    lo = np.asarray(G.bbox_min, F32); hi = np.asarray(G.bbox_max, F32)
    e = F32(0.25) * (hi - lo).max()
    base = scene.make_rays_incoherent(lo - e, hi + e, 8192, SEED + 10)
    cat, fam = H.catalogue(tris, G, mesh=False)
    return np.ascontiguousarray(np.concatenate([base, cat]), F32), np.concatenate([np.full(8192, "0"), fam])


# ---- scenes that are refused ------------------------------------------------------------------------------------------------------------------

EINVAL, ERANGE = "EINVAL", "ERANGE"


def clean_soup():
    return scene.make_soup(500)


def nonfinite_scenes():
    """[(name, tris, expected answer)]: the 500-triangle soup with one NaN, +inf or -inf in v0, e1, e2 or a normal component of the first, the 7th or the
    last triangle; all triangles NaN; finite vertices at +-3e38, whose extent overflows (refused as a range, not as an argument)."""
    base = clean_soup()
    out = []
    columns = {"v0": 1, "e1": 4, "e2": 10, "n": 7}
    for vname, value in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for cname, col in columns.items():
            for pname, row in (("first", 0), ("7th", 6), ("last", 499)):
                t = base.copy(); t[row, col] = F32(value)
                out.append((f"{vname}-{cname}-{pname}", t, EINVAL, row))
    out.append(("all-nan", np.full_like(base, np.nan), EINVAL, None))
    far = np.array([[-3e38, 0, 0], [3e38, 0, 0]], F32)
    t = base.copy()
    t[3:5] = scene.tris_from_vertices(far, far + F32([0, 1, 0]), far + F32([0, 0, 1]))
    assert np.isfinite(t).all()
    out.append(("extent-overflow", t, ERANGE, None))
    return out


# ---- reference totals in 64 bits ----------------------------------------------------------------------------------------------------------------

def top_level(tris, top_density=TOP_DENSITY):
    """(dims, lo, hi) of the top-level grid as hagrid_build_grid computes it, from the L0 functions of the oracle (float32 throughout)"""
    import ctypes as C
    from oracle import oracle as O
    L = O.lib()
    lo, hi = scene.tris_bbox(tris)
    bb = O.OBBox(); bb.min[:] = [float(x) for x in lo]; bb.max[:] = [float(x) for x in hi]
    if not L.orc_grid_dims_defined(C.byref(bb), tris.shape[0], C.c_float(top_density)):
        wb = O.OBBox(); L.orc_widen_scene_box(C.byref(bb), C.byref(wb)); bb = wb
    d = (C.c_int * 3)()
    L.orc_compute_grid_dims(C.byref(bb), tris.shape[0], C.c_float(top_density), d)
    dims = np.array([x + (x & 1) for x in d], np.int64)
    lo = np.array(list(bb.min), F32); hi = np.array(list(bb.max), F32)
    ext = (hi - lo).astype(F32)
    return dims, (lo - ext * F32(0.001)).astype(F32), (hi + ext * F32(0.001)).astype(F32)


def top_reference_total(tris, top_density=TOP_DENSITY) -> int:
    """the number of (primitive, top-level cell) pairs, count_new_refs summed in 64 bits: compute_range restated in float32 with numpy"""
    dims, lo, hi = top_level(tris, top_density)
    v0 = tris[:, 0:3]; v1 = v0 - tris[:, 4:7]; v2 = v0 + tris[:, 8:11]
    bmin = np.minimum(v0, np.minimum(v1, v2)); bmax = np.maximum(v0, np.maximum(v1, v2))
    inv = (dims.astype(F32) / (hi - lo)).astype(F32)
    l = np.maximum(((bmin - lo) * inv).astype(F32).astype(np.int64), 0)
    h = np.minimum(((bmax - lo) * inv).astype(F32).astype(np.int64), dims - 1)
    return int(np.maximum(np.prod(h - l + 1, axis=1), 0).sum())


def slabs(n, width, thickness, seed):
    """n triangles that each cover a width x width square in a slab of the given thickness: a top-level grid of many cells in x and y and two in z"""
    u = _u(seed, n, 3)
    c = np.stack([u[:, 0] * F32(1 - width), u[:, 1] * F32(1 - width), u[:, 2] * F32(thickness)], axis=1).astype(F32)
    w = F32(width)
    v1 = c + np.array([w, 0, 0], F32); v2 = c + np.array([0, w, 0], F32)
    # the hypotenuse spans the square: the triangle's box is the square
    return scene.tris_from_vertices(c, v1, v2)


def size_scenes():
    """[(band, tris)]: thin slabs whose true top-level reference total lies in (2^30, 2^31), in (2^31, 2^32), and above 2^32 with its low 32 bits
    inside (0, 2^30) -- the total a 32-bit sum would accept.  The tests compute the totals and assert the bands."""
    return [("a", slabs(3000, 1.0, 1e-6, 20)), ("b", slabs(4096, 1.0, 1e-6, 21)), ("c", slabs(6000, 1.0, 1e-6, 22))]


BANDS = {"a": lambda t: 2 ** 30 < t < 2 ** 31, "b": lambda t: 2 ** 31 < t < 2 ** 32, "c": lambda t: t > 2 ** 32 and 0 < t % 2 ** 32 < 2 ** 30}
