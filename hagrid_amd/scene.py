"""Synthetic scenes and ray buffers.

Everything is generated from a counter-based 64-bit integer PRNG (splitmix64 finaliser keyed by
``seed + (index + 1) * golden``), so any machine produces identical bits and any slice of a buffer
can be generated independently (rank ``r`` of a multi-GPU run generates only its own rays).
No libm, no ``numpy.random``.

Layouts follow the reference PODs:
  Tri  = 12 x f32: v0.xyz, n.x, e1.xyz, n.y, e2.xyz, n.z   (prims.h:13-25, main.cpp:259-267)
  Ray  =  8 x f32: org.xyz, tmin, dir.xyz, tmax           (ray.h:9-20)
  Hit  = {i32 id, f32 t, f32 u, f32 v}                     (ray.h:22-33)
"""
from __future__ import annotations

import numpy as np

HIT_DTYPE = np.dtype([("id", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])
CELL_DTYPE = np.dtype([("min", "<i4", 3), ("begin", "<i4"), ("max", "<i4", 3), ("end", "<i4")])
SMALL_CELL_DTYPE = np.dtype([("min", "<u2", 3), ("max", "<u2", 3), ("begin", "<i4")])
# nearest-surface queries (hagrid_closest_points): 16 bytes in, 32 bytes out per query
POINT_QUERY_DTYPE = np.dtype([("p", "<f4", 3), ("r", "<f4")])
CLOSEST_DTYPE = np.dtype([("q", "<f4", 3), ("d2", "<f4"), ("id", "<i4"), ("feature", "<i4"), ("side", "<f4"), ("zero", "<i4")])
# neighbour queries (hagrid_nearest_tris): 8 bytes per slot of a list, and per cursor
NEAREST_ENTRY_DTYPE = np.dtype([("d2", "<f4"), ("id", "<i4")])
# capsule queries (hagrid_segment_tris): 32 bytes per segment; a record is CLOSEST_DTYPE with s in the word that is 0 there
SEGMENT_DTYPE = np.dtype([("a", "<f4", 3), ("r", "<f4"), ("b", "<f4", 3), ("pad", "<f4")])
SEGMENT_RECORD_DTYPE = np.dtype([("q", "<f4", 3), ("d2", "<f4"), ("id", "<i4"), ("feature", "<i4"), ("side", "<f4"), ("s", "<f4")])
# box-overlap queries (hagrid_overlap_boxes): 32 bytes per box, the layout of BBox with `first` in the pad slot after min
BOX_QUERY_DTYPE = np.dtype([("min", "<f4", 3), ("first", "<i4"), ("max", "<f4", 3), ("pad", "<i4")])
OVERLAP_ANY = 1
OBB_DTYPE = np.dtype([("c", "<f4", 3), ("first", "<i4"), ("u", "<f4", 3), ("pad_u", "<i4"), ("v", "<f4", 3), ("pad_v", "<i4"), ("w", "<f4", 3), ("pad_w", "<i4")])

FLT_MAX = np.float32(3.4028234663852886e38)

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)

SCENE_SEED_BASE = 0x48414752494400  # + N          
RAY_SEED_BASE = 0x52415953          # + config #


def _mix(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def uniform01(seed: int, index: np.ndarray) -> np.ndarray:
    """float32 in [0,1): (splitmix64(seed, index) >> 40) * 2^-24."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (index.astype(np.uint64) + np.uint64(1)) * _GOLDEN
        z = _mix(z)
    return ((z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def _cross(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    # vec.h:104-109 in float32, no fused ops
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(np.float32)


def tris_from_vertices(v0: np.ndarray, v1: np.ndarray, v2: np.ndarray) -> np.ndarray:
    """Pack triangles exactly like main.cpp:259-267: e1 = v0 - v1, e2 = v2 - v0, n = cross(e1, e2)."""
    v0 = v0.astype(np.float32); v1 = v1.astype(np.float32); v2 = v2.astype(np.float32)
    e1 = v0 - v1
    e2 = v2 - v0
    n = _cross(e1, e2)
    out = np.empty((v0.shape[0], 12), dtype=np.float32)
    out[:, 0:3] = v0; out[:, 3] = n[:, 0]
    out[:, 4:7] = e1; out[:, 7] = n[:, 1]
    out[:, 8:11] = e2; out[:, 11] = n[:, 2]
    return out


def make_soup(num_tris: int, seed: int | None = None, first: int = 0, count: int | None = None) -> np.ndarray:
    """Scene "soup-N": c ~ U[0,1)^3, a, b ~ U[-s, s]^3, s = N^(-1/3); v0 = c, v1 = c + a, v2 = c + b."""
    if seed is None:
        seed = SCENE_SEED_BASE + num_tris
    if count is None:
        count = num_tris - first
    s = np.float32(float(num_tris) ** (-1.0 / 3.0))
    idx = (np.arange(first, first + count, dtype=np.uint64)[:, None] * np.uint64(9)
           + np.arange(9, dtype=np.uint64)[None, :])
    u = uniform01(seed, idx)
    c = u[:, 0:3]
    a = (np.float32(2.0) * u[:, 3:6] - np.float32(1.0)) * s
    b = (np.float32(2.0) * u[:, 6:9] - np.float32(1.0)) * s
    return tris_from_vertices(c, c + a, c + b)


def make_clustered(num_sparse: int = 100000, clusters: int = 6, per_cluster: int = 150000) -> np.ndarray:
    """A very non-uniform scene (teapot in a stadium, the case irregular grids exist for): a sparse soup over the unit cube
    and `clusters` dense blobs, each a soup shrunk to 4 % of the cube.  With the defaults: 1M triangles, grid shift 6, cell
    lists of up to ~20 references inside the blobs.  Normals are recomputed from the scaled edges as make_soup does."""
    parts = [make_soup(num_sparse, seed=7)]
    for k in range(clusters):
        c = make_soup(per_cluster, seed=20 + k).copy()
        centre = np.float32([0.15 + 0.14 * k, 0.3 + 0.08 * k, 0.2 + 0.1 * k])
        c[:, 0:3] = c[:, 0:3] * np.float32(0.04) + centre
        c[:, 4:7] *= np.float32(0.03); c[:, 8:11] *= np.float32(0.03)
        n = _cross(c[:, 4:7], c[:, 8:11]).astype(np.float32)
        c[:, 3] = n[:, 0]; c[:, 7] = n[:, 1]; c[:, 11] = n[:, 2]
        parts.append(c)
    return np.ascontiguousarray(np.concatenate(parts), np.float32)


def make_gradient(num_tris: int = 1_000_000, seed: int | None = None) -> np.ndarray:
    """A soup whose density rises towards one corner: positions squared, edges scaled with the local stretch.  Long tiles of many cells with short lists -- the
    scene family on which counting iterations mispredicts what four lanes per ray buy (profiles/NOTES.md "Round 5")."""
    base = make_soup(num_tris, seed=seed)
    v0 = base[:, 0:3].astype(np.float64); e1 = -base[:, 4:7].astype(np.float64); e2 = base[:, 8:11].astype(np.float64)      # v1 = v0 - e1, v2 = v0 + e2 (prims.h)
    k = np.maximum(2.0 * v0, 0.05); v0 = v0 ** 2
    return tris_from_vertices(v0.astype(np.float32), (v0 + e1 * k).astype(np.float32), (v0 + e2 * k).astype(np.float32))


def make_shell(num_tris: int = 1_000_000, seed: int | None = None) -> np.ndarray:
    """A surface: the soup's triangles moved onto a sphere of radius 0.4, nothing inside or around it."""
    base = make_soup(num_tris, seed=seed)
    v0 = base[:, 0:3].astype(np.float64); e1 = -base[:, 4:7].astype(np.float64); e2 = base[:, 8:11].astype(np.float64)
    d = v0 - 0.5; d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6); v0 = 0.5 + 0.4 * d
    return tris_from_vertices(v0.astype(np.float32), (v0 + e1).astype(np.float32), (v0 + e2).astype(np.float32))


def _sincos_turns(turns: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """sin and cos of 2 pi * turns in float64 from + and x only (octant reduction, Taylor series): any machine produces identical bits (no libm)."""
    t = np.asarray(turns, np.float64); t = t - np.floor(t)
    q = np.floor(t * 8.0 + 0.5)                       # nearest multiple of an eighth turn
    x = (t - q / 8.0) * 6.283185307179586             # |x| <= pi / 8
    x2 = x * x
    s = x * (1.0 + x2 * (-1.0 / 6 + x2 * (1.0 / 120 + x2 * (-1.0 / 5040 + x2 * (1.0 / 362880 + x2 * (-1.0 / 39916800 + x2 * (1.0 / 6227020800)))))))
    c = 1.0 + x2 * (-0.5 + x2 * (1.0 / 24 + x2 * (-1.0 / 720 + x2 * (1.0 / 40320 + x2 * (-1.0 / 3628800 + x2 * (1.0 / 479001600 + x2 * (-1.0 / 87178291200)))))))
    r = 0.7071067811865476
    sq = np.array([0.0, r, 1.0, r, 0.0, -r, -1.0, -r])[q.astype(np.int64) % 8]; cq = np.array([1.0, r, 0.0, -r, -1.0, -r, 0.0, r])[q.astype(np.int64) % 8]
    return sq * c + cq * s, cq * c - sq * s


def _grid_faces(nu: int, nv: int, wrap_u: bool, wrap_v: bool, base: int) -> np.ndarray:
    """two triangles per quad of an nu x nv vertex lattice (vertex (i, j) = base + i * nv + j), wrapping where asked: shared vertices, no duplicates"""
    iu = np.arange(nu if wrap_u else nu - 1); jv = np.arange(nv if wrap_v else nv - 1)
    i, j = np.meshgrid(iu, jv, indexing="ij"); i = i.ravel(); j = j.ravel()
    i1 = (i + 1) % nu; j1 = (j + 1) % nv
    a = base + i * nv + j; b = base + i1 * nv + j; c = base + i1 * nv + j1; d = base + i * nv + j1
    return np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


def make_stadium_mesh(detail: float = 1.0, solids_only: bool = False):
    """"Teapot in a stadium" (the reference README's own motivation, README.md:5-12) as an INDEXED mesh: finely tessellated connected surfaces -- tori and
    spheres with shared vertices, a grain of dust among them -- inside a hall of ten huge triangles, with terraces of long thin ones and pillars of slivers as
    high as the hall.  With detail = 1: ~0.96M triangles whose edges span four orders of magnitude (1.0 ... 1e-4).  Returns (vertices float32 [nv, 3], faces
    int32 [nf, 3], zero-based); write_obj() / tris_from_mesh() take it from there.  `detail` scales the tessellation (tests use small ones).
    solids_only: only the CLOSED surfaces -- the four tori, the three spheres and the three lamps, without the hall, the terraces, the pillars and the dust
    (make_closed_solids) -- and a third return value: each solid's analytic description, a dict with kind ("torus" | "sphere"), centre, radii (R, r of a
    torus; (r,) of a sphere), tilt (turns about the x axis; 0 for a sphere) and faces (first face, number of faces)."""
    V = []; F = []; nvert = 0; solids = []

    def add(verts, faces):
        nonlocal nvert
        V.append(np.asarray(verts, np.float64)); F.append(np.asarray(faces, np.int32)); nvert += len(verts)

    # the hall: floor, ceiling, two side walls, back wall of the unit cube (open towards the camera at -z): 8 shared corners, 10 triangles of edge 1
    open_parts = not solids_only          # the hall, the terraces, the pillars and the dust
    if open_parts:
        corners = [[x, y, z] for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)]
        quads = [(0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5), (4, 5, 7, 6)]
        add(corners, [[nvert + q[0], nvert + q[1], nvert + q[2]] for q in quads] + [[nvert + q[0], nvert + q[2], nvert + q[3]] for q in quads])
    # terraces along the back wall: a staircase profile swept across x (treads and risers 0.9 long, 0.03 deep)
    if open_parts:
        steps = 12
        prof = [(0.0 + 0.03 * ((k + 1) // 2), 0.97 - 0.03 * (k // 2)) for k in range(2 * steps + 1)]          # (y, z) of the profile's corners
        tv = [[x, y, z] for (y, z) in prof for x in (0.05, 0.95)]
        add(tv, _grid_faces(len(prof), 2, False, False, nvert))
    # pillars: coarse cylinders from floor to ceiling, 16 segments: slivers 1.0 high and 0.004 wide
    for k in range(8 if open_parts else 0):
        cx, cz = (0.12 if k % 2 == 0 else 0.88), 0.15 + 0.2 * (k // 2)
        sn, cs = _sincos_turns(np.arange(16) / 16.0)
        ring = [[cx + 0.01 * c, y, cz + 0.01 * s_] for c, s_ in zip(cs, sn) for y in (0.0, 1.0)]
        add(ring, _grid_faces(16, 2, True, False, nvert))

    def torus(centre, R, r, nu, nv, tilt):
        u = np.arange(nu) / nu; v = np.arange(nv) / nv
        su, cu = _sincos_turns(u); sv, cv = _sincos_turns(v); st, ct = _sincos_turns(np.array([tilt]))
        solids.append({"kind": "torus", "centre": tuple(centre), "radii": (R, r), "tilt": tilt, "faces": (sum(len(f) for f in F), 2 * nu * nv)})
        x = (R + r * cv[None, :]) * cu[:, None]; z = (R + r * cv[None, :]) * su[:, None]; y = np.broadcast_to(r * sv[None, :], x.shape)
        y2 = y * ct[0] - z * st[0]; z2 = y * st[0] + z * ct[0]                                   # tilted about the x axis
        add(np.stack([x + centre[0], y2 + centre[1], z2 + centre[2]], -1).reshape(-1, 3), _grid_faces(nu, nv, True, True, nvert))

    def sphere(centre, r, nu, nv):
        # nu meridians x (nv - 1) rings between two pole vertices (fans at the poles: no degenerate triangles)
        u = np.arange(nu) / nu; lat = np.arange(1, nv) / (2.0 * nv)                              # turns from the north pole, (0, 1/2)
        solids.append({"kind": "sphere", "centre": tuple(centre), "radii": (r,), "tilt": 0.0, "faces": (sum(len(f) for f in F), 2 * nu * (nv - 1))})
        su, cu = _sincos_turns(u); sl, cl = _sincos_turns(lat)
        x = r * sl[None, :] * cu[:, None]; z = r * sl[None, :] * su[:, None]; y = np.broadcast_to(r * cl[None, :], x.shape)
        base = nvert
        body = np.stack([x + centre[0], y + centre[1], z + centre[2]], -1).reshape(-1, 3)
        faces = _grid_faces(nu, nv - 1, True, False, base)
        north, south = base + nu * (nv - 1), base + nu * (nv - 1) + 1
        i = np.arange(nu); i1 = (i + 1) % nu
        fans = np.concatenate([np.stack([np.full(nu, north), base + i1 * (nv - 1), base + i * (nv - 1)], 1),
                               np.stack([np.full(nu, south), base + i * (nv - 1) + nv - 2, base + i1 * (nv - 1) + nv - 2], 1)]).astype(np.int32)
        add(np.concatenate([body, [[centre[0], centre[1] + r, centre[2]], [centre[0], centre[1] - r, centre[2]]]]), np.concatenate([faces, fans]))

    d = lambda n: max(8, int(round(n * detail)))
    for k, (c, tilt) in enumerate([((0.30, 0.12, 0.35), 0.0), ((0.68, 0.15, 0.40), 0.07), ((0.45, 0.30, 0.62), 0.19), ((0.60, 0.10, 0.25), 0.31)]):
        torus(c, 0.08, 0.03, d(400), d(200), tilt)                                               # 4 x 160k triangles, edge ~1.3e-3
    for c in ((0.40, 0.06, 0.20), (0.75, 0.30, 0.65), (0.22, 0.25, 0.55)):
        sphere(c, 0.05, d(300), d(150))                                                          # 3 x 90k, edge ~1e-3
    if open_parts:
        sphere((0.50, 0.02, 0.30), 0.004, d(200), d(100))                                        # a grain of dust: 40k triangles, edge ~1e-4
    for c in ((0.2, 0.8, 0.5), (0.5, 0.85, 0.7), (0.8, 0.8, 0.45)):
        sphere(c, 0.1, 16, 8)                                                                    # lamps: coarse, edge ~0.04
    if solids_only:
        return np.concatenate(V).astype(np.float32), np.concatenate(F).astype(np.int32), solids
    return np.concatenate(V).astype(np.float32), np.concatenate(F).astype(np.int32)


def make_closed_solids(detail: float = 1.0) -> tuple[np.ndarray, list]:
    """(triangles, solids): the closed surfaces of make_stadium_mesh -- four tori, three spheres, three lamps -- in face order, and their analytic
    descriptions: the scene whose inside / outside is known (solid_distance)."""
    verts, faces, solids = make_stadium_mesh(detail, solids_only=True)
    return tris_from_mesh(verts, faces), solids


def solid_distance(solid: dict, points: np.ndarray) -> np.ndarray:
    """signed distance (float64, negative inside) of points (n, 3) to the ANALYTIC surface of one solid of make_closed_solids"""
    p = np.asarray(points, np.float64)[:, 0:3] - np.asarray(solid["centre"], np.float64)
    if solid["kind"] == "sphere":
        return np.sqrt((p * p).sum(axis=1)) - solid["radii"][0]
    st, ct = _sincos_turns(np.array([solid["tilt"]]))
    y = p[:, 1] * ct[0] + p[:, 2] * st[0]; z = -p[:, 1] * st[0] + p[:, 2] * ct[0]            # back into the torus's own frame (axis y)
    R, r = solid["radii"]
    ring = np.sqrt(p[:, 0] * p[:, 0] + z * z) - R
    return np.sqrt(ring * ring + y * y) - r


def tris_from_mesh(verts: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """the triangles of an indexed mesh as main.cpp:259-267 packs them (v0, e1 = v0 - v1, e2 = v2 - v0, n)"""
    return np.ascontiguousarray(tris_from_vertices(verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]))


def transform_points(M: np.ndarray, v: np.ndarray) -> np.ndarray:
    """Points v (n, 3) under the 3 x 4 matrix M (12 floats, row-major, last column = translation) in float32, one rounding per operation, in
    the order include/hagrid/assemble.h writes it: x' = ((M[0]*x + M[1]*y) + M[2]*z) + M[3], rows 1 and 2 likewise with M[4..7], M[8..11]."""
    M = np.asarray(M, dtype=np.float32).reshape(12)
    v = np.asarray(v, dtype=np.float32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] for r in range(3)], axis=1).astype(np.float32)


def assemble_tris(meshes, instance_mesh=None, transforms=None) -> tuple[np.ndarray, np.ndarray, int]:
    """The Tri array of a scene of indexed meshes and instances -- the numpy statement of hagrid_scene_assemble (include/hagrid_amd.h), bit for bit.
    meshes: a list of (vertices, faces): vertices float32 (V, >= 3) (columns beyond the third are padding: a stride of 16 bytes is a (V, 4)
    array), faces int32 (F, 3), or None for F = V // 3 triangles on the vertices 3p, 3p+1, 3p+2 -- or (vertices, None, F) to say F.
    instance_mesh: the mesh every instance places (None: one instance per mesh, in order).  transforms: (I, 12) or (I, 3, 4) float32, or None (the
    vertices as they are).  Instances are laid out in order, each with its mesh's triangles in mesh order.  A triangle that names a vertex
    outside its mesh becomes the degenerate triangle on the mesh's vertex 0 and is counted.
    Returns (tris (N, 12) float32, origins (N, 2) int32 = (instance, triangle within its mesh), number of such triangles)."""
    if instance_mesh is None:
        instance_mesh = range(len(meshes))
    instance_mesh = [int(k) for k in instance_mesh]
    if transforms is not None:
        transforms = np.asarray(transforms, dtype=np.float32).reshape(len(instance_mesh), 12)
    tris, origins, bad = [np.empty((0, 12), np.float32)], [np.empty((0, 2), np.int32)], 0
    for i, k in enumerate(instance_mesh):
        verts = np.asarray(meshes[k][0], dtype=np.float32)[:, 0:3]
        faces = meshes[k][1]
        if faces is None:
            count = int(meshes[k][2]) if len(meshes[k]) > 2 else verts.shape[0] // 3
            faces = np.arange(3 * count, dtype=np.int64).reshape(count, 3)
        faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
        if faces.shape[0] == 0:
            continue
        wrong = ((faces < 0) | (faces >= verts.shape[0])).any(axis=1)
        faces = np.where(wrong[:, None], 0, faces)
        bad += int(wrong.sum())
        if transforms is not None:
            verts = transform_points(transforms[i], verts)
        tris.append(tris_from_vertices(verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]))
        origins.append(np.stack([np.full(faces.shape[0], i), np.arange(faces.shape[0])], axis=1).astype(np.int32))
    return np.ascontiguousarray(np.concatenate(tris), np.float32), np.ascontiguousarray(np.concatenate(origins), np.int32), bad


def make_stadium(detail: float = 1.0) -> np.ndarray:
    """the triangles of make_stadium_mesh(), in face order"""
    return tris_from_mesh(*make_stadium_mesh(detail))


def write_obj(path: str, verts: np.ndarray, faces: np.ndarray, mixed_forms: bool = True) -> None:
    """An indexed mesh as a Wavefront OBJ file the reference's loader reads (load_obj.cpp:78-239): vertices with nine significant digits (a float32 survives the
    round trip), one-based faces; with mixed_forms every third face is written as v/vt/vn and every third with negative indices."""
    nv = verts.shape[0]
    with open(path, "w") as f:
        f.write("# hagrid_amd.scene.write_obj\nvt 0 0\nvn 0 0 1\n")
        f.write("".join("v %.9g %.9g %.9g\n" % (float(x), float(y), float(z)) for x, y, z in verts.astype(np.float64)))
        a = faces.astype(np.int64) + 1
        lines = []
        for k in range(0, a.shape[0], 1 << 16):
            blk = a[k:k + (1 << 16)]
            for i, (p, q, r) in enumerate(blk, start=k):
                m = i % 3 if mixed_forms else 0
                if m == 0: lines.append("f %d %d %d\n" % (p, q, r))
                elif m == 1: lines.append("f %d/1/1 %d/1/1 %d/1/1\n" % (p, q, r))
                else: lines.append("f %d %d %d\n" % (p - nv - 1, q - nv - 1, r - nv - 1))
            f.write("".join(lines)); lines = []


def make_rays_aimed(bbox_min, bbox_max, num_rays: int, seed: int, first: int = 0) -> np.ndarray:
    """Incoherent origins (make_rays_incoherent) with directions towards the blobs of make_clustered, with some spread: ray i aims at blob i % 6.  The rays
    that end inside the dense parts of a very non-uniform scene (bench.py --config clustered --rays aimed; tests/test_fullsize_gpu.py)."""
    rays = make_rays_incoherent(bbox_min, bbox_max, num_rays, seed, first=first).copy()
    k = (np.arange(first, first + num_rays) % 6).astype(np.float32)
    centre = np.stack([np.float32(0.17) + np.float32(0.14) * k, np.float32(0.32) + np.float32(0.08) * k, np.float32(0.22) + np.float32(0.1) * k], axis=1).astype(np.float32)
    rays[:, 4:7] = centre - rays[:, 0:3] + np.float32(0.02) * rays[:, 4:7]
    return np.ascontiguousarray(rays, np.float32)


def tris_bbox(tris: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Scene bounding box over the three vertices (prims.h:27-31)."""
    v0 = tris[:, 0:3]; v1 = v0 - tris[:, 4:7]; v2 = v0 + tris[:, 8:11]
    lo = np.minimum(v0, np.minimum(v1, v2)).min(axis=0)
    hi = np.maximum(v0, np.maximum(v1, v2)).max(axis=0)
    return lo.astype(np.float32), hi.astype(np.float32)


def make_rays_incoherent(bbox_min, bbox_max, num_rays: int, seed: int, first: int = 0,
                         tmin: float = 0.0, tmax: float = float(FLT_MAX)) -> np.ndarray:
    """org ~ U(bbox); dir rejection-sampled from U[-1,1]^3 with 0.01 < |d|^2 <= 1, un-normalised."""
    lo = np.asarray(bbox_min, dtype=np.float32); hi = np.asarray(bbox_max, dtype=np.float32)
    ids = np.arange(first, first + num_rays, dtype=np.uint64)
    rays = np.empty((num_rays, 8), dtype=np.float32)
    uo = uniform01(seed, ids[:, None] * np.uint64(3) + np.arange(3, dtype=np.uint64)[None, :])
    rays[:, 0:3] = lo + uo * (hi - lo)
    rays[:, 3] = np.float32(tmin)
    rays[:, 7] = np.float32(tmax)
    todo = np.arange(num_rays)
    dseed = seed ^ 0x6469720000000000
    for attempt in range(64):
        if todo.size == 0:
            break
        base = (ids[todo] * np.uint64(64) + np.uint64(attempt)) * np.uint64(3)
        u = uniform01(dseed, base[:, None] + np.arange(3, dtype=np.uint64)[None, :])
        d = np.float32(2.0) * u - np.float32(1.0)
        l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        ok = (l2 > np.float32(0.01)) & (l2 <= np.float32(1.0))
        rays[todo[ok], 4:7] = d[ok]
        todo = todo[~ok]
    if todo.size:
        rays[todo, 4:7] = np.float32([0.0, 0.0, 1.0])
    return rays


def camera(bbox_min, bbox_max, eye_dist: float = 0.8, fov: float = 60.0, ratio: float = 1.0, yaw: float = 0.0, strafe: float = 0.0):
    """gen_camera (main.cpp:42-50) looking down +z at the bbox centre from eye_dist * diagonal away.  yaw (radians) turns the view about the
    up axis and strafe (scene diagonals) moves the eye sideways: what the reference's viewer does per mouse pixel (0.005 rad) and per key
    event (0.005 x the scene size), main.cpp:579-586 -- a frame loop with a moving camera (tools/dev_moving_camera.py, bench.py)."""
    lo = np.asarray(bbox_min, dtype=np.float32); hi = np.asarray(bbox_max, dtype=np.float32)
    ext = hi - lo
    diag = np.float32(np.sqrt(np.float32(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2])))
    center = np.float32(0.5) * (hi + lo)
    eye = (center + np.float32([0.0, 0.0, -1.0]) * np.float32(eye_dist) * diag).astype(np.float32)
    up0 = np.float32([0.0, 1.0, 0.0])
    if yaw or strafe:
        eye = (eye + np.float32([1.0, 0.0, 0.0]) * np.float32(strafe) * diag).astype(np.float32)
        fwd = np.float32([np.sin(yaw), 0.0, np.cos(yaw)])
        center = (eye + fwd * np.float32(eye_dist) * diag).astype(np.float32)

    def norm(v):
        return (v * (np.float32(1.0) / np.float32(np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))))).astype(np.float32)

    def cross(a, b):
        return np.float32([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    f = np.float32(np.tan(np.pi * fov / 360.0))
    cdir = norm(center - eye)
    right = norm(cross(cdir, up0)) * np.float32(f * np.float32(ratio))
    up = norm(cross(right, cdir)) * f
    return eye, cdir, right.astype(np.float32), up.astype(np.float32), diag


def make_rays_primary(bbox_min, bbox_max, width: int, height: int, first: int = 0, count: int | None = None,
                      eye_dist: float = 0.8, fov: float = 60.0, sample: int = 0, num_samples: int = 1, yaw: float = 0.0, strafe: float = 0.0) -> np.ndarray:
    """gen_rays (main.cpp:52-66): pixel (x, y) -> dir = cam.dir + right*kx + up*ky, tmax = clip = |extents|.
    sample / num_samples shifts the pixel by a sub-pixel offset in x (sample 0 of 1 = the reference's rays):
    the weak-scaling batches of a multi-GPU run are the N sub-pixel samples of the same camera."""
    eye, cdir, right, up, diag = camera(bbox_min, bbox_max, eye_dist, fov, width / float(height), yaw, strafe)
    if count is None:
        count = width * height - first
    pid = np.arange(first, first + count, dtype=np.int64)
    x = (pid % width).astype(np.float32); y = (pid // width).astype(np.float32)
    if sample:
        x = x + np.float32(sample) / np.float32(num_samples)
    kx = np.float32(2.0) * x / np.float32(width) - np.float32(1.0)
    ky = np.float32(1.0) - np.float32(2.0) * y / np.float32(height)
    rays = np.empty((count, 8), dtype=np.float32)
    rays[:, 0:3] = eye
    rays[:, 3] = np.float32(0.0)
    rays[:, 4:7] = cdir[None, :] + right[None, :] * kx[:, None] + up[None, :] * ky[:, None]
    rays[:, 7] = diag
    return rays


def make_rays_inactive(num_rays: int) -> np.ndarray:
    """Rays with an empty interval (org = 0, dir = (0,0,1), tmin = 0, tmax = -1): traversal answers id -1, t -1."""
    out = np.zeros((num_rays, 8), dtype=np.float32)
    out[:, 6] = np.float32(1.0); out[:, 7] = np.float32(-1.0)
    return out


def make_rays_bounce(tris: np.ndarray, rays: np.ndarray, hits: np.ndarray, bbox_min, bbox_max, seed: int,
                     first: int = 0, tmax: float = float(FLT_MAX), redraw_misses: bool = True) -> np.ndarray:
    """Diffuse-bounce rays (BASELINE config 5): from each hit, org = p + 1e-4 * n, cosine-weighted
    direction about the ray-facing normal from two PRNG floats keyed by the ray index, tmax as given; misses are
    re-drawn as incoherent rays (tmax = FLT_MAX), or with redraw_misses=False become inactive rays (make_rays_inactive).
    The device form is hagrid_gen_bounce_rays (include/hagrid/frame.h: bounce_ray), bit for bit."""
    n_rays = rays.shape[0]
    hid = hits["id"]
    if redraw_misses:
        out = make_rays_incoherent(bbox_min, bbox_max, n_rays, seed ^ 0x6D69737300000000, first)
    else:
        out = make_rays_inactive(n_rays)
    hit_mask = hid >= 0
    if not hit_mask.any():
        return out
    r = rays[hit_mask]; t = hits["t"][hit_mask]
    tri = tris[hid[hit_mask]]
    p = r[:, 0:3] + r[:, 4:7] * t[:, None]
    n = np.stack([tri[:, 3], tri[:, 7], tri[:, 11]], axis=1)
    ln = np.sqrt(np.maximum((n * n).sum(axis=1), np.float32(1e-30))).astype(np.float32)
    n = n / ln[:, None]
    facing = (n * r[:, 4:7]).sum(axis=1) > 0
    n[facing] = -n[facing]
    ids = np.arange(first, first + n_rays, dtype=np.uint64)[hit_mask]
    u = uniform01(seed, ids[:, None] * np.uint64(2) + np.arange(2, dtype=np.uint64)[None, :])
    # cosine-weighted hemisphere via a polynomial-free construction: disk point by rejection-free
    # concentric mapping would need trig; use (r, phi) with sqrt only and a rational unit circle
    # parametrisation phi -> ((1-s^2)/(1+s^2), 2s/(1+s^2)), s in [-1,1), mirrored by the second bit.
    s = np.float32(2.0) * u[:, 1] - np.float32(1.0)
    half = (ids & np.uint64(1)).astype(np.float32) * np.float32(2.0) - np.float32(1.0)
    cx = (np.float32(1.0) - s * s) / (np.float32(1.0) + s * s) * half
    cy = np.float32(2.0) * s / (np.float32(1.0) + s * s)
    rad = np.sqrt(u[:, 0]).astype(np.float32)
    dx = rad * cx; dy = rad * cy
    dz = np.sqrt(np.maximum(np.float32(1.0) - u[:, 0], np.float32(0.0))).astype(np.float32)
    # orthonormal basis (Frisvad-free, branch on the dominant axis)
    a = np.where((np.abs(n[:, 0]) > np.float32(0.5))[:, None], np.float32([0.0, 1.0, 0.0])[None, :], np.float32([1.0, 0.0, 0.0])[None, :]).astype(np.float32)
    tx = _cross(a, n)
    tx = tx / np.sqrt((tx * tx).sum(axis=1)).astype(np.float32)[:, None]
    ty = _cross(n, tx)
    d = tx * dx[:, None] + ty * dy[:, None] + n * dz[:, None]
    b = np.empty((r.shape[0], 8), dtype=np.float32)
    b[:, 0:3] = p + np.float32(1e-4) * n
    b[:, 3] = np.float32(0.0)
    b[:, 4:7] = d
    b[:, 7] = np.float32(tmax)
    out[hit_mask] = b
    return out.astype(np.float32)


SHADE_DEPTH, SHADE_GRAY, SHADE_HEAT = 0, 1, 2
_GRADIENT = np.float32([[0, 0, 255], [0, 255, 255], [0, 128, 0], [255, 255, 0], [255, 0, 0]])      # R G B (main.cpp:69-75)


def shade_hits(hits: np.ndarray, mode: int, clip: float = 0.0) -> np.ndarray:
    """update_surface (main.cpp:68-111) in float32: (n, 4) uint8, B G R A with A = 255.  The device form is hagrid_shade_hits.
    DEPTH: uint8(min(255 * t / clip, 255)) (negative values give 0); GRAY: uint8(min(255, id)), so -1 wraps to 255 as the reference's
    uint8_t does; HEAT: the five-colour gradient of min(100, max(id, 0)) / 100."""
    n = hits.shape[0]
    out = np.empty((n, 4), dtype=np.uint8)
    out[:, 3] = 255
    hid = hits["id"].astype(np.int32)
    if mode == SHADE_DEPTH:
        if not clip > 0:
            raise ValueError("the depth picture needs clip > 0")
        v = np.float32(255.0) * hits["t"].astype(np.float32) / np.float32(clip)
        v = np.minimum(np.maximum(v, np.float32(0.0)), np.float32(255.0))
        out[:, 0:3] = v.astype(np.uint8)[:, None]
    elif mode == SHADE_GRAY:
        out[:, 0:3] = (np.minimum(255, hid) & 255).astype(np.uint8)[:, None]
    elif mode == SHADE_HEAT:
        k = np.minimum(100, np.maximum(hid, 0)).astype(np.float32) / np.float32(100.0)
        s = np.float32(1.0) / np.float32(5.0)
        i = np.minimum(4, (k * np.float32(5.0)).astype(np.int32))
        j = np.minimum(4, i + 1)
        t = ((k - i.astype(np.float32) * s) / s).astype(np.float32)
        c = (np.float32(1.0) - t)[:, None] * _GRADIENT[i] + t[:, None] * _GRADIENT[j]
        out[:, 0] = c[:, 2].astype(np.uint8); out[:, 1] = c[:, 1].astype(np.uint8); out[:, 2] = c[:, 0].astype(np.uint8)
    else:
        raise ValueError(f"unknown shading mode {mode}")
    return out


def shade_layers(hits: np.ndarray, k: int, clip: float, opacity: float) -> np.ndarray:
    """The picture of sorted hit lists (traverse_grid_multi: hits of shape (n, k) or (n * k,), HIT_DTYPE) in float32: every slot with id >= 0
    is a layer of the given opacity in its depth colour min(max(255 * t / clip, 0), 255), composited front to back over white:
    acc = 0, T = 1; per layer acc = acc + (T * opacity) * c, T = T * (1 - opacity); then acc = acc + T * 255; B = G = R = uint8(min(acc, 255)),
    A = 255.  The device form is hagrid_shade_layers, the per-pixel function shade_layers of include/hagrid/frame.h."""
    if not clip > 0:
        raise ValueError("the depth colours need clip > 0")
    if not 0 < opacity <= 1:
        raise ValueError("opacity must be in (0, 1]")
    h = np.asarray(hits).reshape(-1, k)
    op = np.float32(opacity)
    acc = np.zeros(h.shape[0], dtype=np.float32); T = np.ones(h.shape[0], dtype=np.float32)
    for j in range(k):
        on = h["id"][:, j] >= 0
        with np.errstate(over="ignore"):          # an unused slot holds tmax, often FLT_MAX: its colour is computed and not used
            c = np.float32(255.0) * h["t"][:, j].astype(np.float32) / np.float32(clip)
        c = np.minimum(np.maximum(c, np.float32(0.0)), np.float32(255.0))
        acc = np.where(on, acc + (T * op) * c, acc).astype(np.float32)
        T = np.where(on, T * (np.float32(1.0) - op), T).astype(np.float32)
    acc = acc + T * np.float32(255.0)
    out = np.empty((h.shape[0], 4), dtype=np.uint8)
    out[:, 0:3] = np.minimum(acc, np.float32(255.0)).astype(np.uint8)[:, None]
    out[:, 3] = 255
    return out


def shade_occlusion(hits: np.ndarray, counts: np.ndarray, samples: int) -> np.ndarray:
    """The ambient-occlusion picture: B=G=R = 255 * (samples - counts) // samples where the PRIMARY hit has id >= 0, else 0; A = 255.
    counts: how many of a pixel's `samples` occlusion rays were blocked (clamped to 0 .. samples).  The device form is hagrid_shade_occlusion."""
    if samples <= 0:
        raise ValueError("samples must be positive")
    c = np.clip(np.asarray(counts, np.int64), 0, samples)
    v = np.where(hits["id"] >= 0, 255 * (samples - c) // samples, 0).astype(np.uint8)
    out = np.empty((hits.shape[0], 4), dtype=np.uint8)
    out[:, 0:3] = v[:, None]; out[:, 3] = 255
    return out


# ---- point batches for nearest-surface queries (counter-based like the ray generators: no libm, the same bits everywhere) ---------------

def _uniform_rows(seed: int, count: int, width: int) -> np.ndarray:
    idx = np.arange(count, dtype=np.uint64)[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)[None, :]
    return uniform01(seed, idx)


def bbox_diagonal(bbox_min, bbox_max) -> np.float32:
    e = (np.asarray(bbox_max, np.float32) - np.asarray(bbox_min, np.float32)).astype(np.float32)
    return np.float32(np.sqrt(np.float32(np.float32(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])))


def make_points_surface(tris: np.ndarray, count: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """(points on triangles, their triangle): the triangle uniform by index, barycentrics folded into the triangle; float32, operations in the order written"""
    u = _uniform_rows(seed, count, 3)
    j = np.minimum((u[:, 0] * np.float32(tris.shape[0])).astype(np.int64), tris.shape[0] - 1)
    a, b = u[:, 1], u[:, 2]
    fold = a + b > np.float32(1.0)
    a = np.where(fold, np.float32(1.0) - a, a); b = np.where(fold, np.float32(1.0) - b, b)
    t = tris[j]
    p = t[:, 0:3] - t[:, 4:7] * a[:, None] + t[:, 8:11] * b[:, None]          # v0 + a (v1 - v0) + b (v2 - v0)
    return p.astype(np.float32), j


def make_gaussian3(seed: int, count: int) -> np.ndarray:
    """(count, 3) float32, close to N(0, 1): the sum of twelve uniforms minus six"""
    u = _uniform_rows(seed, count * 3, 12)
    s = u[:, 0]
    for k in range(1, 12):
        s = s + u[:, k]
    return (s - np.float32(6.0)).reshape(count, 3).astype(np.float32)


def make_points_uniform(bbox_min, bbox_max, count: int, seed: int, enlarge: float = 0.1) -> np.ndarray:
    """uniform in the box enlarged by `enlarge` of its extents (half on every side)"""
    lo = np.asarray(bbox_min, np.float32); hi = np.asarray(bbox_max, np.float32)
    ext = hi - lo
    a = lo - np.float32(0.5 * enlarge) * ext; e = ext * np.float32(1.0 + enlarge)
    return (a + _uniform_rows(seed, count, 3) * e).astype(np.float32)


def make_points_near_surface(tris: np.ndarray, bbox_min, bbox_max, count: int, seed: int, sigma: float = 0.01) -> np.ndarray:
    """surface samples moved by a Gaussian of `sigma` box diagonals per axis"""
    p, _ = make_points_surface(tris, count, seed)
    return (p + make_gaussian3(seed ^ 0x67617573, count) * (np.float32(sigma) * bbox_diagonal(bbox_min, bbox_max))).astype(np.float32)


# ---- nearest-surface queries: the numpy statement of include/hagrid/closest.h (same operations, same order, same bits) ------------------

def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub3(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _segment_d2(p, a, ab):
    """segment_d2 of closest.h: (d2, q)"""
    zero, one = np.float32(0.0), np.float32(1.0)
    t = _dot3(_sub3(p, a), ab) / _dot3(ab, ab)
    t = np.where(t > zero, t, zero)
    t = np.where(t < one, t, one)
    q = (a[0] + ab[0] * t, a[1] + ab[1] * t, a[2] + ab[2] * t)
    d = _sub3(p, q)
    return _dot3(d, d), q


def _point_tri(p, T, want_q: bool):
    """point_tri (and tri_side) of closest.h on broadcastable float32 arrays: p = (x, y, z), T = the 12 columns of the Tri records.
    Returns valid, d2 and -- with want_q -- q (three arrays), feature, side."""
    zero = np.float32(0.0)
    v0, e1, e2, n = (T[0], T[1], T[2]), (T[4], T[5], T[6]), (T[8], T[9], T[10]), (T[3], T[7], T[11])
    valid = ~((n[0] == zero) & (n[1] == zero) & (n[2] == zero))
    v1 = _sub3(v0, e1); v2 = (v0[0] + e2[0], v0[1] + e2[1], v0[2] + e2[2])
    u1 = (-e1[0], -e1[1], -e1[2]); u2 = _sub3(v2, v1)
    d2, q = _segment_d2(p, v0, u1)
    f = np.ones(np.shape(d2), dtype=np.int32)
    for k, (a, ab) in ((2, (v1, u2)), (3, (v0, e2))):
        dk, qk = _segment_d2(p, a, ab)
        less = dk < d2
        d2 = np.where(less, dk, d2)
        if want_q:
            q = tuple(np.where(less, qk[i], q[i]) for i in range(3)); f = np.where(less, np.int32(k), f)
    d0 = _sub3(p, v0); d1 = _sub3(p, v1)
    nn = _dot3(n, n)
    s1 = _dot3(_cross3(e1, d0), n); s2 = _dot3(_cross3(d1, u2), n); s3 = _dot3(_cross3(e2, d0), n)
    inside = (s1 >= zero) & (s2 >= zero) & (s3 >= zero) & (nn > zero)
    h = _dot3(d0, n)
    df = h * h / nn
    face = inside & (df <= d2)
    d2 = np.where(face, df, d2)
    if not want_q:
        return valid, d2
    hn = h / nn
    q = tuple(np.where(face, p[i] - n[i] * hn, q[i]) for i in range(3))
    f = np.where(face, np.int32(0), f)
    s = _dot3(_sub3(p, q), n)
    side = np.where(s > zero, np.int32(1), np.where(s < zero, np.int32(-1), np.int32(0)))
    return valid, d2, q, f, side


def closest_pairs(tris: np.ndarray, points: np.ndarray) -> dict:
    """Triangle i against point i (points: (n, 3+) float32): valid (the triangle has a surface), d2, q (n, 3), feature, side -- the per-pair values
    of include/hagrid/closest.h (point_tri, tri_side), bit for bit."""
    T = np.ascontiguousarray(tris, dtype=np.float32); P = np.ascontiguousarray(points, dtype=np.float32)
    with np.errstate(all="ignore"):
        valid, d2, q, f, side = _point_tri((P[:, 0], P[:, 1], P[:, 2]), [T[:, i] for i in range(12)], True)
    return {"valid": valid, "d2": d2.astype(np.float32), "q": np.stack(q, axis=1).astype(np.float32), "feature": f.astype(np.int32), "side": side.astype(np.int32)}


def closest_points(tris: np.ndarray, points: np.ndarray, chunk_pairs: int = 1 << 21) -> np.ndarray:
    """The definition of hagrid_closest_points by brute force: points (n, 4) float32 x, y, z, r (or POINT_QUERY_DTYPE) -> CLOSEST_DTYPE records.
    Among the triangles with a surface (stored normal != 0) and d2 <= r * r the smallest by (d2, id); none: id -1, d2 = r * r, q = p, feature =
    side = 0; r < 0: an inactive query, id -1 and d2 = -1; a NaN coordinate: id -1.  Every point against every triangle, a chunk of points at a time."""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    P = np.ascontiguousarray(points).view(np.float32).reshape(-1, 4)
    n, N = P.shape[0], T.shape[0]
    out = np.zeros(n, dtype=CLOSEST_DTYPE)
    cols = [T[None, :, i] for i in range(12)]
    m = max(1, chunk_pairs // max(N, 1))
    inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        for o in range(0, n, m):
            p = P[o:o + m]
            r2 = p[:, 3] * p[:, 3]
            res = out[o:o + m]
            res["q"] = p[:, 0:3]; res["d2"] = r2; res["id"] = -1
            if N:
                valid, d2 = _point_tri((p[:, 0:1], p[:, 1:2], p[:, 2:3]), cols, False)
                mask = valid & (d2 <= r2[:, None]) & (p[:, 3:4] >= np.float32(0.0))
                d2m = np.where(mask, d2, inf)
                mn = d2m.min(axis=1)
                cand = mask & (d2 == mn[:, None])
                has = cand.any(axis=1)
                win = cand.argmax(axis=1)                          # the first of the tied triangles: the smallest id
                Tw = T[win]
                _, d2w, q, f, side = _point_tri((p[:, 0], p[:, 1], p[:, 2]), [Tw[:, i] for i in range(12)], True)
                assert (d2w[has].view(np.uint32) == mn[has].view(np.uint32)).all()
                res["id"] = np.where(has, win, -1)
                res["d2"] = np.where(has, d2w, r2)
                res["q"] = np.where(has[:, None], np.stack(q, axis=1), p[:, 0:3])
                res["feature"] = np.where(has, f, 0)
                res["side"] = np.where(has, side, 0).astype(np.float32)
            res["d2"] = np.where(p[:, 3] < np.float32(0.0), np.float32(-1.0), res["d2"])
            out[o:o + m] = res
    return out


def _sorted_candidates(T, cols, p, k, cursors, query_labels, tri_labels):
    """the candidates of hagrid_nearest_tris for a chunk of points p (m, 4) as three flat arrays (query, triangle, d2), grouped by query and sorted by
    (d2, id) inside a query; k: None = all of them, else at least the k smallest of every query"""
    r2 = p[:, 3] * p[:, 3]
    if p.shape[1] == 8:                                          # segments: seg_tri, and no walk for a coordinate that is not finite
        valid, d2 = _seg_tri((p[:, 0:1], p[:, 1:2], p[:, 2:3]), (p[:, 4:5], p[:, 5:6], p[:, 6:7]), cols, False)
        valid = valid & np.isfinite(p[:, [0, 1, 2, 4, 5, 6]]).all(axis=1)[:, None]
    else:
        valid, d2 = _point_tri((p[:, 0:1], p[:, 1:2], p[:, 2:3]), cols, False)
    mask = valid & (d2 <= r2[:, None]) & (p[:, 3:4] >= np.float32(0.0))
    if cursors is not None:
        cd, ci = cursors["d2"][:, None], cursors["id"][:, None]
        mask &= (d2 > cd) | ((d2 == cd) & (np.arange(T.shape[0], dtype=np.int64)[None, :] > ci))
    if query_labels is not None:
        for ql in (query_labels[:, None],) if query_labels.ndim == 1 else (query_labels[:, 0:1], query_labels[:, 1:2]):
            mask &= ~((ql >= 0) & ((tri_labels[None, :, 0] == ql) | (tri_labels[None, :, 1] == ql) | (tri_labels[None, :, 2] == ql)))
    if k is not None and T.shape[0] > k:
        kth = np.partition(np.where(mask, d2, np.float32(np.inf)), k - 1, axis=1)[:, k - 1]
        mask &= d2 <= kth[:, None]
    rows, ids = np.nonzero(mask)                                 # by query, ids ascending inside a query
    d = d2[rows, ids]
    order = np.lexsort((d, rows))                                # stable: a tie in d2 keeps the ids ascending
    return rows[order], ids[order], d[order]


def _list_args(tris, queries, width, cursors, query_labels, tri_labels):
    """the arguments of a list query as arrays; width: 4 floats per query (a point, one label) or 8 (a segment, two labels)"""
    assert (query_labels is None) == (tri_labels is None), "query_labels and tri_labels are given together or not at all"
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    Q = np.ascontiguousarray(queries).view(np.float32).reshape(-1, width)
    C_ = None if cursors is None else np.ascontiguousarray(cursors).view(NEAREST_ENTRY_DTYPE).reshape(-1)
    ql = None if query_labels is None else np.asarray(query_labels, dtype=np.int32).reshape((-1,) if width == 4 else (-1, 2))
    tl = None if tri_labels is None else np.asarray(tri_labels, dtype=np.int32).reshape(-1, 3)
    return T, Q, C_, ql, tl


def _k_lists(tris, queries, width, record_dtype, k, cursors, query_labels, tri_labels, chunk_pairs):
    """nearest_tris (width 4, CLOSEST_DTYPE) and segment_tris (width 8, SEGMENT_RECORD_DTYPE): every query against every triangle, a chunk of queries at a
    time; the k smallest candidates by rank; the records made again from the winners"""
    T, Q, C_, ql, tl = _list_args(tris, queries, width, cursors, query_labels, tri_labels)
    n, N = Q.shape[0], T.shape[0]
    k = int(k)
    entries = np.zeros((n, k), dtype=NEAREST_ENTRY_DTYPE)
    records = np.zeros((n, k), dtype=record_dtype)
    cols = [T[None, :, i] for i in range(12)]
    m = max(1, chunk_pairs // max(N, 1))
    with np.errstate(all="ignore"):
        r2 = Q[:, 3] * Q[:, 3]
        entries["d2"] = np.where(Q[:, 3] < np.float32(0.0), np.float32(-1.0), r2)[:, None]
        entries["id"] = -1
        for o in range(0, n if N else 0, m):
            s = slice(o, o + m)
            rows, ids, d = _sorted_candidates(T, cols, Q[s], k, None if C_ is None else C_[s], None if ql is None else ql[s], tl)
            start = np.searchsorted(rows, rows)                  # the first position of each entry's query
            rank = np.arange(rows.size) - start
            keep = rank < k
            entries["id"][o + rows[keep], rank[keep]] = ids[keep]
            entries["d2"][o + rows[keep], rank[keep]] = d[keep]
        records["q"] = Q[:, None, 0:3]; records["d2"] = entries["d2"]; records["id"] = entries["id"]
        qi, sj = np.nonzero(entries["id"] >= 0)
        if qi.size:
            Tw = T[entries["id"][qi, sj]]; p = Q[qi]
            Tc = [Tw[:, i] for i in range(12)]
            if width == 8:
                _, d2w, q, f, side, sw = _seg_tri((p[:, 0], p[:, 1], p[:, 2]), (p[:, 4], p[:, 5], p[:, 6]), Tc, True)
                records["s"][qi, sj] = sw
            else:
                _, d2w, q, f, side = _point_tri((p[:, 0], p[:, 1], p[:, 2]), Tc, True)
            assert (d2w.astype(np.float32).view(np.uint32) == entries["d2"][qi, sj].view(np.uint32)).all()
            records["q"][qi, sj] = np.stack(q, axis=1); records["feature"][qi, sj] = f; records["side"][qi, sj] = side.astype(np.float32)
    return entries, records


def _all_lists(tris, queries, width, query_labels, tri_labels, chunk_pairs) -> dict:
    """tris_within (width 4) and tris_near_segments (width 8): every candidate of every query, sorted, in CSR form"""
    T, Q, _, ql, tl = _list_args(tris, queries, width, None, query_labels, tri_labels)
    n, N = Q.shape[0], T.shape[0]
    counts = np.zeros(n, dtype=np.int64)
    all_ids, all_d = [np.zeros(0, np.int32)], [np.zeros(0, np.float32)]
    cols = [T[None, :, i] for i in range(12)]
    m = max(1, chunk_pairs // max(N, 1))
    with np.errstate(all="ignore"):
        for o in range(0, n if N else 0, m):
            s = slice(o, o + m)
            rows, ids, d = _sorted_candidates(T, cols, Q[s], None, None, None if ql is None else ql[s], tl)
            np.add.at(counts, o + rows, 1)
            all_ids.append(ids.astype(np.int32)); all_d.append(d.astype(np.float32))
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return {"offsets": offsets, "ids": np.concatenate(all_ids), "d2": np.concatenate(all_d)}


def nearest_tris(tris: np.ndarray, points: np.ndarray, k: int, cursors=None, query_labels=None, tri_labels=None, chunk_pairs: int = 1 << 21):
    """The definition of hagrid_nearest_tris by brute force: points (n, 4) float32 x, y, z, r (or POINT_QUERY_DTYPE).  Triangle j is a candidate of query i
    when it has a surface (stored normal != 0), d2 <= r * r (a NaN d2 never is), the pair is not skipped by the labels (query_labels (n,) int32, tri_labels
    (N, 3) int32, both or neither: skipped when query_labels[i] >= 0 equals one of tri_labels[j]) and (d2, j) sorts strictly after cursors[i]
    (NEAREST_ENTRY_DTYPE (n,), or None) in the order (d2 ascending, id ascending).  Returns (entries (n, k) NEAREST_ENTRY_DTYPE, records (n, k)
    CLOSEST_DTYPE): the k smallest candidates in that order; unused slots id -1, d2 = r * r, q = p; r < 0: an inactive query, every slot id -1 and
    d2 = -1.  Every point against every triangle, a chunk of points at a time."""
    return _k_lists(tris, points, 4, CLOSEST_DTYPE, k, cursors, query_labels, tri_labels, chunk_pairs)


def tris_within(tris: np.ndarray, points: np.ndarray, query_labels=None, tri_labels=None, chunk_pairs: int = 1 << 21) -> dict:
    """ALL the candidates of nearest_tris (no cursor) of every point, sorted by (d2, id), in CSR form: "offsets" int64 (n + 1,), "ids" int32 and "d2"
    float32 (total,) -- what the pages of hagrid_nearest_tris concatenate to (api.tris_within).  For queries with a finite radius: r = inf lists every
    triangle of the scene."""
    return _all_lists(tris, points, 4, query_labels, tri_labels, chunk_pairs)


# ---- ball lists, stages 2 and 3: the numpy statement of include/hagrid/unique_lists.h ----------------------------------------------

def _segment_ranges(offsets, capacity: int):
    """the room rule of hagrid_list_crossings for CSR segments: (first, room) per segment"""
    off = np.asarray(offsets, dtype=np.int64)
    b, e = off[:-1], off[1:]
    ok = (b >= 0) & (e >= b) & (e <= int(capacity))
    return np.where(ok, b, 0), np.where(ok, e - b, 0)


def empty_entry() -> np.ndarray:
    e = np.zeros((), dtype=NEAREST_ENTRY_DTYPE)
    e["d2"] = np.float32(np.inf); e["id"] = -1
    return e


def unique_lists(offsets, entries: np.ndarray, capacity=None):
    """The definition of hagrid_unique_lists: every segment [offsets[i], offsets[i + 1]) of entries (NEAREST_ENTRY_DTYPE (capacity,)) -- entries with id < 0 or a
    NaN d2 dropped, the rest sorted by (d2 by float comparison, id), equal ids reduced to one (equal ids carry equal d2 bits: the contract), the survivors at
    the front, (+inf, -1) in every other slot.  Returns (the entries afterwards, counts int32 (n,)); slots outside every segment are unchanged."""
    out = np.ascontiguousarray(entries).view(NEAREST_ENTRY_DTYPE).reshape(-1).copy()
    cap = out.size if capacity is None else int(capacity)
    first, room = _segment_ranges(offsets, cap)
    counts = np.zeros(first.size, dtype=np.int32)
    for i in range(first.size):
        seg = out[first[i]:first[i] + room[i]]
        with np.errstate(invalid="ignore"):
            v = seg[(seg["id"] >= 0) & ~np.isnan(seg["d2"])]
        # (d2 + 0 turns -0.0 into +0.0: the sort key is the float VALUE; the bits that travel are the entry's own)
        v = v[np.lexsort((v["id"], v["d2"] + np.float32(0.0)))]
        if v.size:
            v = v[np.concatenate([[True], v["id"][1:] != v["id"][:-1]])]
        seg[:v.size] = v
        seg[v.size:] = empty_entry()
        counts[i] = v.size
    return out, counts


def compact_lists(offsets, entries: np.ndarray, counts, out_offsets, out_capacity: int, capacity=None, fill=None) -> np.ndarray:
    """The definition of hagrid_compact_lists: out_entries (out_capacity,) -- the first min(counts[i], room of the source, room of the destination) entries of
    segment i at out_offsets[i], (+inf, -1) in the rest of the destination's room; slots outside every destination segment keep `fill` (None: zero bytes)."""
    src = np.ascontiguousarray(entries).view(NEAREST_ENTRY_DTYPE).reshape(-1)
    cap = src.size if capacity is None else int(capacity)
    out = np.zeros(int(out_capacity), dtype=NEAREST_ENTRY_DTYPE) if fill is None else np.ascontiguousarray(fill).view(NEAREST_ENTRY_DTYPE).reshape(-1).copy()
    first, room = _segment_ranges(offsets, cap)
    dfirst, droom = _segment_ranges(out_offsets, int(out_capacity))
    for i in range(first.size):
        c = max(0, min(int(counts[i]), int(room[i]), int(droom[i])))
        out[dfirst[i]:dfirst[i] + c] = src[first[i]:first[i] + c]
        out[dfirst[i] + c:dfirst[i] + droom[i]] = empty_entry()
    return out


# ---- capsule queries: the numpy statement of include/hagrid/capsule.h (same operations, same order, same bits) ---------------------------

def _clamp01(x):
    zero, one = np.float32(0.0), np.float32(1.0)
    x = np.where(x > zero, x, zero)
    return np.where(x < one, x, one)


def _seg_edge(a, d, A, e, u):
    """seg_edge of capsule.h: (d2, q, s) of the segment a + d * s against the edge e + u * t"""
    zero, one = np.float32(0.0), np.float32(1.0)
    d2_0, q_0 = _segment_d2(a, e, u)                               # A == 0: the candidate IS segment_d2
    w = _sub3(a, e)
    E = _dot3(u, u); F = _dot3(u, w); C = _dot3(d, w)
    B = _dot3(d, u)
    den = A * E - B * B
    s = np.where(den > zero, _clamp01((B * F - C * E) / den), zero)
    t = (B * s + F) / E
    s_lo = _clamp01(-C / A); s_hi = _clamp01((B - C) / A)
    lo = ~(t >= zero); hi = ~lo & (t > one)
    s = np.where(lo, s_lo, np.where(hi, s_hi, s)); t = np.where(lo, zero, np.where(hi, one, t))
    flat = E == zero                                               # an edge of no length
    s = np.where(flat, s_lo, s); t = np.where(flat, zero, t)
    c = tuple(a[i] + d[i] * s for i in range(3))
    q = tuple(e[i] + u[i] * t for i in range(3))
    cq = _sub3(c, q)
    d2 = _dot3(cq, cq)
    point = A == zero
    return np.where(point, d2_0, d2), tuple(np.where(point, q_0[i], q[i]) for i in range(3)), np.where(point, zero, s)


def _seg_tri(a, b, T, want_q: bool):
    """seg_tri (and tri_side) of capsule.h on broadcastable float32 arrays: a, b = (x, y, z), T = the 12 columns of the Tri records.
    Returns valid, d2 and -- with want_q -- q (three arrays), feature, side, s."""
    zero, one = np.float32(0.0), np.float32(1.0)
    v0, e1, e2, n = (T[0], T[1], T[2]), (T[4], T[5], T[6]), (T[8], T[9], T[10]), (T[3], T[7], T[11])
    valid, d2, q, f, _ = _point_tri(a, T, True)
    _, db, qb, fb, _ = _point_tri(b, T, True)
    shape = np.broadcast(d2, db).shape
    less = db < d2
    d2 = np.where(less, db, d2); q = tuple(np.where(less, qb[i], q[i]) for i in range(3)); f = np.where(less, fb, f)
    s = np.where(less, one, np.zeros(shape, np.float32))
    v1 = _sub3(v0, e1); v2 = (v0[0] + e2[0], v0[1] + e2[1], v0[2] + e2[2])
    u1 = (-e1[0], -e1[1], -e1[2]); u2 = _sub3(v2, v1)
    d = _sub3(b, a)
    A = _dot3(d, d)
    for k, (e, u) in ((1, (v0, u1)), (2, (v1, u2)), (3, (v0, e2))):
        dk, qk, sk = _seg_edge(a, d, A, e, u)
        less = dk < d2
        d2 = np.where(less, dk, d2)
        if want_q:
            q = tuple(np.where(less, qk[i], q[i]) for i in range(3)); f = np.where(less, np.int32(k), f); s = np.where(less, sk, s)
    ha = _dot3(_sub3(a, v0), n); hb = _dot3(_sub3(b, v0), n)
    cross_ = ((ha > zero) & (hb < zero)) | ((ha < zero) & (hb > zero))
    sx = ha / (ha - hb)
    x = tuple(a[i] + d[i] * sx for i in range(3))
    x0 = _sub3(x, v0); x1 = _sub3(x, v1)
    s1 = _dot3(_cross3(e1, x0), n); s2 = _dot3(_cross3(x1, u2), n); s3 = _dot3(_cross3(e2, x0), n)
    pierce = cross_ & (s1 >= zero) & (s2 >= zero) & (s3 >= zero) & (_dot3(n, n) > zero) & (zero < d2)
    d2 = np.where(pierce, zero, d2)
    if not want_q:
        return valid, d2
    q = tuple(np.where(pierce, x[i], q[i]) for i in range(3)); f = np.where(pierce, np.int32(4), f); s = np.where(pierce, sx, s)
    c = tuple(a[i] + d[i] * s for i in range(3))
    sd = _dot3(_sub3(c, q), n)
    side = np.where(sd > zero, np.int32(1), np.where(sd < zero, np.int32(-1), np.int32(0)))
    return valid, d2, q, f, side, s


def _segments(segments) -> np.ndarray:
    return np.ascontiguousarray(segments).view(np.float32).reshape(-1, 8)


def segment_pairs(tris: np.ndarray, segments: np.ndarray) -> dict:
    """Triangle i against segment i (segments: (n, 8) float32 ax, ay, az, r, bx, by, bz, 0, or SEGMENT_DTYPE): valid (the triangle has a surface), d2,
    q (n, 3) on the triangle, feature (0 face, 1 .. 3 edge, 4 pierced), side, s -- the per-pair values of include/hagrid/capsule.h (seg_tri, tri_side),
    bit for bit."""
    T = np.ascontiguousarray(tris, dtype=np.float32); S = _segments(segments)
    with np.errstate(all="ignore"):
        valid, d2, q, f, side, s = _seg_tri((S[:, 0], S[:, 1], S[:, 2]), (S[:, 4], S[:, 5], S[:, 6]), [T[:, i] for i in range(12)], True)
    return {"valid": valid, "d2": d2.astype(np.float32), "q": np.stack(q, axis=1).astype(np.float32), "feature": f.astype(np.int32),
            "side": side.astype(np.int32), "s": s.astype(np.float32)}


def segment_tris(tris: np.ndarray, segments: np.ndarray, k: int, cursors=None, query_labels=None, tri_labels=None, chunk_pairs: int = 1 << 20):
    """The definition of hagrid_segment_tris by brute force: segments (n, 8) float32 ax, ay, az, r, bx, by, bz, 0 (or SEGMENT_DTYPE).  Triangle j is a
    candidate of query i when it has a surface, seg_tri's d2 <= r * r (a NaN d2 never is), the pair is not skipped by the labels (query_labels (n, 2)
    int32, tri_labels (N, 3) int32, both or neither: skipped when one of query_labels[i] >= 0 equals one of tri_labels[j]) and (d2, j) sorts strictly
    after cursors[i] (NEAREST_ENTRY_DTYPE (n,), or None).  Returns (entries (n, k) NEAREST_ENTRY_DTYPE, records (n, k) SEGMENT_RECORD_DTYPE): the k
    smallest candidates by (d2, id); unused slots id -1, d2 = r * r, q = a, s = 0; r < 0: an inactive query, every slot id -1 and d2 = -1; a NaN or
    infinite coordinate: id -1, d2 = r * r.  Every segment against every triangle, a chunk of segments at a time."""
    return _k_lists(tris, segments, 8, SEGMENT_RECORD_DTYPE, k, cursors, query_labels, tri_labels, chunk_pairs)


def tris_near_segments(tris: np.ndarray, segments: np.ndarray, query_labels=None, tri_labels=None, chunk_pairs: int = 1 << 20) -> dict:
    """ALL the candidates of segment_tris (no cursor) of every segment, sorted by (d2, id), in CSR form: "offsets" int64 (n + 1,), "ids" int32 and "d2"
    float32 (total,) -- what the pages of hagrid_segment_tris concatenate to (api.tris_near_segments).  For queries with a finite radius."""
    return _all_lists(tris, segments, 8, query_labels, tri_labels, chunk_pairs)


def mesh_edges(faces: np.ndarray) -> np.ndarray:
    """the unique edges of an indexed mesh as (m, 2) int32 vertex pairs, smaller index first, sorted"""
    F = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    e = np.sort(e, axis=1)
    return np.unique(e[e[:, 0] != e[:, 1]], axis=0).astype(np.int32)


def make_segments(a, b, r) -> np.ndarray:
    """(n, 8) float32 segment records from ends a, b (n, 3) and radii r (n,) or a scalar"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    s = np.zeros((a.shape[0], 8), dtype=np.float32)
    s[:, 0:3] = a; s[:, 3] = r; s[:, 4:7] = b
    return s


def make_segments_short(tris: np.ndarray, bbox_min, bbox_max, count: int, seed: int, length: float = 0.005, r=np.inf) -> np.ndarray:
    """the ordinary case: a near the surface (make_points_near_surface), b = a + a Gaussian of `length` box diagonals per axis"""
    a = make_points_near_surface(tris, bbox_min, bbox_max, count, seed)
    b = (a + make_gaussian3(seed ^ 0x73686F72, count) * (np.float32(length) * bbox_diagonal(bbox_min, bbox_max))).astype(np.float32)
    return make_segments(a, b, r)


def make_segments_diagonal(bbox_min, bbox_max, count: int, seed: int, r=np.inf) -> np.ndarray:
    """long diagonals: from near one corner of the box to near the opposite one (each end within 5 % of the extents of its corner), the four body
    diagonals in turn"""
    lo = np.asarray(bbox_min, np.float32); hi = np.asarray(bbox_max, np.float32)
    u = _uniform_rows(seed, count, 6) * np.float32(0.05)
    corner = ((np.arange(count)[:, None] % 4) >> np.arange(3)[None, :]) & 1            # x, y flip with the diagonal; z runs low to high
    corner[:, 2] = 0
    ta = np.where(corner == 1, np.float32(1.0) - u[:, 0:3], u[:, 0:3]).astype(np.float32)
    tb = np.where(corner == 1, u[:, 3:6], np.float32(1.0) - u[:, 3:6]).astype(np.float32)
    return make_segments(lo + (hi - lo) * ta, lo + (hi - lo) * tb, r)


def make_segments_axis(bbox_min, bbox_max, count: int, seed: int, r=np.inf) -> np.ndarray:
    """axis-aligned: a uniform in the box, b = a moved along axis i % 3 by up to 30 % of that extent, either way"""
    lo = np.asarray(bbox_min, np.float32); hi = np.asarray(bbox_max, np.float32)
    a = make_points_uniform(lo, hi, count, seed, enlarge=0.0)
    u = _uniform_rows(seed ^ 0x61786973, count, 1)[:, 0]
    b = a.copy()
    axis = np.arange(count) % 3
    b[np.arange(count), axis] = a[np.arange(count), axis] + (u * np.float32(0.6) - np.float32(0.3)) * (hi - lo)[axis]
    return make_segments(a, b, r)


def make_segments_on_edges(tris: np.ndarray, count: int, seed: int, r=np.inf) -> np.ndarray:
    """along triangle edges and on them: for a triangle uniform by index its edge v0 -> v1 (v1 = v0 - e1): a third of the segments the edge itself, a
    third a part of it (a = v0 + u * t0, b = v0 + u * t1), a third the edge moved along the stored normal by 1e-3 of its length (parallel, off the edge)"""
    u = _uniform_rows(seed, count, 3)
    j = np.minimum((u[:, 0] * np.float32(tris.shape[0])).astype(np.int64), tris.shape[0] - 1)
    t = tris[j]
    v0 = t[:, 0:3]; e = (-t[:, 4:7]).astype(np.float32)
    kind = np.arange(count) % 3
    t0 = np.where(kind == 1, u[:, 1], np.float32(0.0))[:, None]; t1 = np.where(kind == 1, u[:, 2], np.float32(1.0))[:, None]
    n = t[:, [3, 7, 11]]
    nn = np.sqrt((n * n).sum(axis=1, dtype=np.float32))[:, None]
    el = np.sqrt((e * e).sum(axis=1, dtype=np.float32))[:, None]
    with np.errstate(all="ignore"):
        off = np.where((kind == 2)[:, None] & (nn > 0), n / nn * (el * np.float32(1e-3)), np.float32(0.0)).astype(np.float32)
    return make_segments(v0 + e * t0 + off, v0 + e * t1 + off, r)


def make_segments_piercing(tris: np.ndarray, bbox_min, bbox_max, count: int, seed: int, r=np.inf) -> np.ndarray:
    """through a face near its centroid: for a triangle uniform by index, from c + w * h to c - w * h with c the centroid, h = 0.5 % of the box
    diagonal and w the unit normal tilted by a Gaussian of 0.2"""
    u = _uniform_rows(seed, count, 1)
    j = np.minimum((u[:, 0] * np.float32(tris.shape[0])).astype(np.int64), tris.shape[0] - 1)
    t = tris[j]
    c = (t[:, 0:3] + (t[:, 8:11] - t[:, 4:7]) * np.float32(1.0 / 3.0)).astype(np.float32)
    n = t[:, [3, 7, 11]]
    nn = np.sqrt((n * n).sum(axis=1, dtype=np.float32))[:, None]
    with np.errstate(all="ignore"):
        w = np.where(nn > 0, n / nn, np.float32([0.0, 0.0, 1.0])).astype(np.float32) + make_gaussian3(seed ^ 0x70696572, count) * np.float32(0.2)
    h = np.float32(0.005) * bbox_diagonal(bbox_min, bbox_max)
    return make_segments(c + w * h, c - w * h, r)


def make_segments_outside(bbox_min, bbox_max, count: int, seed: int, r=np.inf) -> np.ndarray:
    """one end outside the grid (even rows: a uniform in the box, b up to half a diagonal beyond one face) and both outside (odd rows: a and b beyond
    faces of different axes, so some cross the box and some pass it)"""
    lo = np.asarray(bbox_min, np.float32); hi = np.asarray(bbox_max, np.float32)
    diag = bbox_diagonal(lo, hi)
    a = make_points_uniform(lo, hi, count, seed, enlarge=0.0); b = make_points_uniform(lo, hi, count, seed ^ 0x6F757473, enlarge=0.0)
    u = _uniform_rows(seed ^ 0x62657961, count, 2) * np.float32(0.5) * diag + np.float32(0.01) * diag
    i = np.arange(count)
    ax_b = i % 3; up_b = (i // 3) % 2 == 0
    b[i, ax_b] = np.where(up_b, hi[ax_b] + u[:, 0], lo[ax_b] - u[:, 0])
    both = i % 2 == 1
    ax_a = (i + 1) % 3; up_a = (i // 2) % 2 == 0
    a[i, ax_a] = np.where(both, np.where(up_a, hi[ax_a] + u[:, 1], lo[ax_a] - u[:, 1]), a[i, ax_a])
    return make_segments(a, b, r)


# ---- box-overlap queries: the numpy statement of include/hagrid/overlap.h (same operations, same order, same truth values) ----------------

def _edge_axis_separates(A, half, e, f, a, b):
    """edge_axis_separates<A> of prims.h"""
    if A == 0:
        p0 = e[1] * a[2] - e[2] * a[1]; p1 = e[1] * b[2] - e[2] * b[1]; rad = f[2] * half[1] + f[1] * half[2]
    elif A == 1:
        p0 = e[2] * a[0] - e[0] * a[2]; p1 = e[2] * b[0] - e[0] * b[2]; rad = f[2] * half[0] + f[0] * half[2]
    else:
        p0 = e[0] * a[1] - e[1] * a[0]; p1 = e[0] * b[1] - e[1] * b[0]; rad = f[1] * half[0] + f[0] * half[1]
    return (np.fmin(p0, p1) > rad) | (np.fmax(p0, p1) < -rad)


def _tri_box(T, lo, hi):
    """intersect_tri_box<true, true> of prims.h on broadcastable float32 arrays: T = the 12 columns of the Tri records, lo / hi = (x, y, z)"""
    zero, half_ = np.float32(0.0), np.float32(0.5)
    v0, e1, e2, n = (T[0], T[1], T[2]), (T[4], T[5], T[6]), (T[8], T[9], T[10]), (T[3], T[7], T[11])
    near = tuple(np.where(n[i] > zero, lo[i], hi[i]) for i in range(3))
    far = tuple(np.where(n[i] <= zero, lo[i], hi[i]) for i in range(3))
    d = _dot3(v0, n)
    s0 = _dot3(n, near) - d
    s1 = _dot3(n, far) - d
    ok = s1 * s0 <= zero
    v1 = _sub3(v0, e1); v2 = (v0[0] + e2[0], v0[1] + e2[1], v0[2] + e2[2])
    for i in range(3):
        ok = ok & ~((np.fmin(v0[i], np.fmin(v1[i], v2[i])) > hi[i]) | (np.fmax(v0[i], np.fmax(v1[i], v2[i])) < lo[i]))
    c = tuple((hi[i] + lo[i]) * half_ for i in range(3)); half = tuple((hi[i] - lo[i]) * half_ for i in range(3))
    w0, w1, w2 = _sub3(v0, c), _sub3(v1, c), _sub3(v2, c)
    e3 = (e1[0] + e2[0], e1[1] + e2[1], e1[2] + e2[2])
    for e, pairs in ((e1, ((w0, w2), (w0, w2), (w1, w2))), (e2, ((w0, w1), (w0, w1), (w1, w2))), (e3, ((w0, w2), (w0, w2), (w0, w1)))):
        f = (np.abs(e[0]), np.abs(e[1]), np.abs(e[2]))
        for A in range(3):
            ok = ok & ~_edge_axis_separates(A, half, e, f, pairs[A][0], pairs[A][1])
    return ok


def _box_rows(boxes) -> np.ndarray:
    return np.ascontiguousarray(boxes).view(np.float32).reshape(-1, 8)


def overlap_pairs(tris: np.ndarray, boxes: np.ndarray) -> np.ndarray:
    """Triangle i against box i (boxes: (n, 8) float32 rows or BOX_QUERY_DTYPE; `first` is not looked at): does the triangle MEET the box -- meets()
    of include/hagrid/overlap.h, that is intersect_tri_box<true, true> of prims.h.  An inactive box (a NaN bound, min > max) meets nothing.  This is the
    pair alone: a query clips its box first (clip_boxes)."""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12); B = _box_rows(boxes)
    lo = (B[:, 0], B[:, 1], B[:, 2]); hi = (B[:, 4], B[:, 5], B[:, 6])
    with np.errstate(all="ignore"):
        active = (lo[0] <= hi[0]) & (lo[1] <= hi[1]) & (lo[2] <= hi[2])
        return _tri_box([T[:, i] for i in range(12)], lo, hi) & active


def grid_box(tris: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The box of the grid that the build makes over these triangles: the scene box enlarged by 0.1 % of its extent on every side (float32, the build's
    expressions)."""
    lo, hi = tris_bbox(tris)
    d = ((hi - lo).astype(np.float32) * np.float32(0.001)).astype(np.float32)
    return (lo - d).astype(np.float32), (hi + d).astype(np.float32)


def clip_boxes(boxes: np.ndarray, grid_lo, grid_hi) -> np.ndarray:
    """Clip of include/hagrid/overlap.h: (n, 8) float32 rows, every box clipped to the grid box grown by eps = 2^-16 of its largest |coordinate|
    (lo = fmax(lo, grid min - eps), hi = fmin(hi, grid max + eps)); `first` is kept.  Inactive boxes (a NaN bound, min > max) stay as they are; a box
    beyond the grid comes out with min > max."""
    glo = np.asarray(grid_lo, np.float32); ghi = np.asarray(grid_hi, np.float32)
    eps = np.float32(max(np.abs(glo).max(), np.abs(ghi).max())) * np.float32(1.52587890625e-05)
    B = _box_rows(boxes).copy()
    with np.errstate(all="ignore"):
        active = (B[:, 0:3] <= B[:, 4:7]).all(axis=1)
        B[active, 0:3] = np.fmax(B[active, 0:3], (glo - eps).astype(np.float32))
        B[active, 4:7] = np.fmin(B[active, 4:7], (ghi + eps).astype(np.float32))
    return B


def overlap_boxes(tris: np.ndarray, boxes: np.ndarray, k: int = 8, chunk_pairs: int = 1 << 21, grid=None) -> dict:
    """The definition of hagrid_overlap_boxes by brute force: every box, clipped (clip_boxes) to the box of the grid the query runs over -- `grid` =
    (min, max), None: grid_box(tris), what the build makes over these triangles --, against every triangle, a chunk of boxes at a time.  With
    S = {j >= first : j meets the clipped box}: "ids" (n, k) int32 = the min(k, |S|) smallest ids ascending, unused slots -1; "counts" = min(|S|, k + 1);
    "sizes" = |S| (what the device does not report).  Inactive boxes and boxes beyond the grid: count 0, ids -1."""
    glo, ghi = grid_box(tris) if grid is None else grid
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12); B = clip_boxes(boxes, glo, ghi)
    n, N = B.shape[0], T.shape[0]
    first = B[:, 3].view(np.int32)
    ids = np.full((n, k), -1, dtype=np.int32); sizes = np.zeros(n, dtype=np.int64)
    cols = [T[None, :, i] for i in range(12)]
    tid = np.arange(N, dtype=np.int64)[None, :]
    m = max(1, chunk_pairs // max(N, 1))
    with np.errstate(all="ignore"):
        for o in range(0, n if N else 0, m):
            b = B[o:o + m]
            lo = (b[:, 0:1], b[:, 1:2], b[:, 2:3]); hi = (b[:, 4:5], b[:, 5:6], b[:, 6:7])
            active = (lo[0] <= hi[0]) & (lo[1] <= hi[1]) & (lo[2] <= hi[2])
            mask = _tri_box(cols, lo, hi) & active & (tid >= first[o:o + m, None])
            sz = mask.sum(axis=1)
            sizes[o:o + m] = sz
            rows, col = np.nonzero(mask)                       # by row, then by id ascending
            pos = np.arange(rows.size) - (np.cumsum(sz) - sz)[rows]
            sel = pos < k
            ids[o + rows[sel], pos[sel]] = col[sel]
    return {"ids": ids, "counts": np.minimum(sizes, k + 1).astype(np.int32), "sizes": sizes}


def lattice_boxes(origin, size, n) -> np.ndarray:
    """The boxes of hagrid_overlap_lattice as BOX_QUERY_DTYPE records, x fastest: voxel c of an axis is [origin + float(c) * size,
    origin + float(c + 1) * size] -- neighbouring voxels share their faces bit for bit; first = 0."""
    origin = np.asarray(origin, np.float32); size = np.asarray(size, np.float32)
    nx, ny, nz = (int(v) for v in n)
    out = np.zeros(nx * ny * nz, dtype=BOX_QUERY_DTYPE)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for a, c in enumerate((x.reshape(-1), y.reshape(-1), z.reshape(-1))):
        out["min"][:, a] = origin[a] + c.astype(np.float32) * size[a]
        out["max"][:, a] = origin[a] + (c + 1).astype(np.float32) * size[a]
    return out


# ---- contact queries: the numpy statement of include/hagrid/tri_tri.h and of the query form of overlap.h (same operations, same order, same truth values) ----

def _tri_tri(A, B):
    """tri_meets of tri_tri.h on broadcastable float32 arrays: A, B = the 12 columns of the Tri records of the pair"""
    def verts(T):
        v0 = (T[0], T[1], T[2])
        return v0, _sub3(v0, (T[4], T[5], T[6])), (v0[0] + T[8], v0[1] + T[9], v0[2] + T[10])

    va, vb = verts(A), verts(B)
    na, nb = (A[3], A[7], A[11]), (B[3], B[7], B[11])
    ea = (_sub3(va[0], va[1]), _sub3(va[2], va[0]), _sub3(va[2], va[1]))
    eb = (_sub3(vb[0], vb[1]), _sub3(vb[2], vb[0]), _sub3(vb[2], vb[1]))

    def separates(ax):
        pa = [_dot3(ax, v) for v in va]; pb = [_dot3(ax, v) for v in vb]
        min_a = np.fmin(pa[0], np.fmin(pa[1], pa[2])); max_a = np.fmax(pa[0], np.fmax(pa[1], pa[2]))
        min_b = np.fmin(pb[0], np.fmin(pb[1], pb[2])); max_b = np.fmax(pb[0], np.fmax(pb[1], pb[2]))
        return (min_a > max_b) | (min_b > max_a)

    axes = [na] + [_cross3(na, e) for e in ea] + [nb] + [_cross3(nb, e) for e in eb] + [_cross3(e, f) for e in ea for f in eb]
    ok = ~separates(axes[0])
    for ax in axes[1:]:
        ok = ok & ~separates(ax)
    return ok


def tri_tri_pairs(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Triangle a[i] against triangle b[i] ((n, 12) float32 Tri rows): do they MEET -- tri_meets of include/hagrid/tri_tri.h, the separating-axis test
    over 17 axes (the two stored normals, the six in-plane edge normals, the nine edge cross products) on the vertices v0, v0 - e1, v0 + e2."""
    A = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 12); B = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        return _tri_tri([A[:, i] for i in range(12)], [B[:, i] for i in range(12)])


def tri_vertices(tris: np.ndarray) -> np.ndarray:
    """(n, 3, 3) float32: v0, v0 - e1, v0 + e2 as Tri::bbox forms them"""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        return np.stack([T[:, 0:3], (T[:, 0:3] - T[:, 4:7]).astype(np.float32), (T[:, 0:3] + T[:, 8:11]).astype(np.float32)], axis=1)


def tris_admissible(tris: np.ndarray) -> np.ndarray:
    """tri_admissible of prims.h: the twelve floats and the two derived vertices are finite"""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    return np.isfinite(T).all(axis=1) & np.isfinite(tri_vertices(T)).all(axis=(1, 2))


def tris_have_surface(tris: np.ndarray) -> np.ndarray:
    """false: the stored normal is (0, 0, 0)"""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    return ~((T[:, 3] == 0) & (T[:, 7] == 0) & (T[:, 11] == 0))


def query_boxes(queries: np.ndarray, grid_lo, grid_hi) -> np.ndarray:
    """query_box of overlap.h: (n, 8) float32 box rows -- the bounding box of every query triangle grown by eps = 2^-16 of the largest |coordinate| of the
    grid box on every side, first = 0; an INACTIVE query (not admissible, or stored normal 0) gets the inactive box min = 1, max = 0.  Not clipped yet."""
    Q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 12)
    glo = np.asarray(grid_lo, np.float32); ghi = np.asarray(grid_hi, np.float32)
    eps = np.float32(max(np.abs(glo).max(), np.abs(ghi).max())) * np.float32(1.52587890625e-05)
    with np.errstate(all="ignore"):
        V = tri_vertices(Q)
        B = np.zeros((Q.shape[0], 8), dtype=np.float32)
        B[:, 0:3] = np.fmin(V[:, 0], np.fmin(V[:, 1], V[:, 2])) - eps
        B[:, 4:7] = np.fmax(V[:, 0], np.fmax(V[:, 1], V[:, 2])) + eps
    off = ~(tris_admissible(Q) & tris_have_surface(Q))
    B[off, 0:3] = np.float32(1.0); B[off, 4:7] = np.float32(0.0)
    return B


def labels_shared(query_labels: np.ndarray, tri_labels: np.ndarray) -> np.ndarray:
    """labels_shared of overlap.h per pair of rows ((n, 3) int32 each): does a label >= 0 of the query equal a label of the triangle?"""
    q = np.asarray(query_labels, np.int32).reshape(-1, 3); t = np.asarray(tri_labels, np.int32).reshape(-1, 3)
    return ((q[:, :, None] >= 0) & (q[:, :, None] == t[:, None, :])).any(axis=(1, 2))


def overlap_tris(tris: np.ndarray, queries: np.ndarray, k: int = 8, first=None, query_labels=None, tri_labels=None, grid=None, chunk_pairs: int = 1 << 21) -> dict:
    """The definition of hagrid_overlap_tris by brute force.  With box(A) = query_boxes, clipped (clip_boxes) to the box of the grid the query runs over
    (`grid` = (min, max), None: grid_box(tris)), S_i = {j >= first[i] : no label >= 0 of query i is a label of triangle j, triangle j has a surface,
    triangle j meets box(A_i) (overlap_pairs), tri_tri_pairs(A_i, triangle j)}: "ids" (n, k) int32 = the min(k, |S|) smallest ids ascending, unused slots
    -1; "counts" = min(|S|, k + 1); "sizes" = |S|.  first: None or (n,) int32; query_labels (n, 3) and tri_labels (N, 3) int32: both or neither.
    Pairs whose bounding intervals miss each other are left out before the tests: the triangle / box test says the same of them."""
    assert (query_labels is None) == (tri_labels is None), "query_labels and tri_labels are given together or not at all"
    glo, ghi = grid_box(tris) if grid is None else grid
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12); Q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 12)
    B = clip_boxes(query_boxes(Q, glo, ghi), glo, ghi)
    n, N = Q.shape[0], T.shape[0]
    first = np.zeros(n, np.int64) if first is None else np.asarray(first).astype(np.int64)
    ids = np.full((n, k), -1, dtype=np.int32); sizes = np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        V = tri_vertices(T)
        tmin = np.fmin(V[:, 0], np.fmin(V[:, 1], V[:, 2])); tmax = np.fmax(V[:, 0], np.fmax(V[:, 1], V[:, 2]))
        surface = tris_have_surface(T)
        tid = np.arange(N, dtype=np.int64)[None, :]
        m = max(1, chunk_pairs // max(N, 1))
        for o in range(0, n if N else 0, m):
            b = B[o:o + m]
            active = (b[:, 0:3] <= b[:, 4:7]).all(axis=1)
            near = ~((tmin[None, :, :] > b[:, None, 4:7]) | (tmax[None, :, :] < b[:, None, 0:3])).any(axis=2)      # the bounds check of the triangle / box test
            near &= active[:, None] & surface[None, :] & (tid >= first[o:o + m, None])
            rows, col = np.nonzero(near)                       # by row, then by id ascending
            if query_labels is not None:
                keep = ~labels_shared(np.asarray(query_labels).reshape(-1, 3)[o + rows], np.asarray(tri_labels).reshape(-1, 3)[col])
                rows, col = rows[keep], col[keep]
            keep = overlap_pairs(T[col], b[rows]) & tri_tri_pairs(Q[o + rows], T[col])
            rows, col = rows[keep], col[keep]
            sz = np.bincount(rows, minlength=b.shape[0])
            sizes[o:o + b.shape[0]] = sz
            pos = np.arange(rows.size) - (np.cumsum(sz) - sz)[rows]
            sel = pos < k
            ids[o + rows[sel], pos[sel]] = col[sel]
    return {"ids": ids, "counts": np.minimum(sizes, k + 1).astype(np.int32), "sizes": sizes}


# ---- oriented-box queries: the numpy statement of include/hagrid/obb.h (same operations, same order, same truth values) ----------------------------

def _obb_rows(obbs) -> np.ndarray:
    return np.ascontiguousarray(obbs).view(np.float32).reshape(-1, 16)


def make_obbs(centres, u, v, w, first=None) -> np.ndarray:
    """OBB_DTYPE records from (n, 3) arrays: the box of record i is centres[i] + a u[i] + b v[i] + g w[i], |a|, |b|, |g| <= 1"""
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    out = np.zeros(c.shape[0], dtype=OBB_DTYPE)
    out["c"] = c; out["u"] = np.asarray(u, np.float32).reshape(-1, 3); out["v"] = np.asarray(v, np.float32).reshape(-1, 3); out["w"] = np.asarray(w, np.float32).reshape(-1, 3)
    if first is not None:
        out["first"] = np.asarray(first, np.int32)
    return out


def make_rotations(seed: int, count: int) -> np.ndarray:
    """(count, 3, 3) float32 rotation matrices (columns: the axes) from normalised quaternions: +, *, / and a correctly rounded square root only"""
    q = np.float32(2.0) * _uniform_rows(seed, count, 4) - np.float32(1.0)
    q[(q * q).sum(axis=1) < np.float32(1e-3)] = np.float32([1, 0, 0, 0])
    q = (q / np.sqrt((q * q).sum(axis=1, dtype=np.float32))[:, None]).astype(np.float32)
    a, b, c, d = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two = np.float32(2.0)
    R = np.stack([np.stack([a * a + b * b - c * c - d * d, two * (b * c - a * d), two * (b * d + a * c)], axis=1),
                  np.stack([two * (b * c + a * d), a * a - b * b + c * c - d * d, two * (c * d - a * b)], axis=1),
                  np.stack([two * (b * d - a * c), two * (c * d + a * b), a * a - b * b - c * c + d * d], axis=1)], axis=1)
    return R.astype(np.float32)


def _unit_rows(x):
    """rows of x scaled to length 1 (float32; a correctly rounded square root)"""
    return (x / np.sqrt((x * x).sum(axis=1, dtype=np.float32))[:, None]).astype(np.float32)


def make_obb_planks(lo, hi, count: int, seed: int) -> np.ndarray:
    """thin diagonal planks: half extents 50 %, 2 %, 2 % of the diagonal, the long axis along one of the four body diagonals of the box, the centre within
    10 % of the extent of the box's centre"""
    lo = np.asarray(lo, np.float32); hi = np.asarray(hi, np.float32)
    diag = bbox_diagonal(lo, hi)
    ext = (hi - lo).astype(np.float32)
    signs = np.float32([[1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1]])[np.arange(count) % 4]
    u = (np.float32(0.5) * ext * signs).astype(np.float32)
    e = np.eye(3, dtype=np.float32)[(np.arange(count) // 4) % 3]
    v = _unit_rows(np.cross(u, e).astype(np.float32)) * (np.float32(0.02) * diag)
    w = _unit_rows(np.cross(u, v).astype(np.float32)) * (np.float32(0.02) * diag)
    c = ((lo + hi) * np.float32(0.5) + (np.float32(0.2) * _uniform_rows(seed, count, 3) - np.float32(0.1)) * ext).astype(np.float32)
    return make_obbs(c, u, v.astype(np.float32), w.astype(np.float32))


def _obb_tri(O, T):
    """obb_meets of obb.h on broadcastable float32 arrays: O = the 16 columns of the box records, T = the 12 columns of the Tri records"""
    c, u, v, w = (O[0], O[1], O[2]), (O[4], O[5], O[6]), (O[8], O[9], O[10]), (O[12], O[13], O[14])
    v0 = (T[0], T[1], T[2]); v1 = _sub3(v0, (T[4], T[5], T[6])); v2 = (v0[0] + T[8], v0[1] + T[9], v0[2] + T[10])
    edges = (_sub3(v0, v1), _sub3(v2, v0), _sub3(v2, v1))

    def separates(L):
        centre = _dot3(L, c)
        radius = (np.abs(_dot3(L, u)) + np.abs(_dot3(L, v))) + np.abs(_dot3(L, w))
        p0, p1, p2 = _dot3(L, v0), _dot3(L, v1), _dot3(L, v2)
        return (np.fmin(p0, np.fmin(p1, p2)) > centre + radius) | (np.fmax(p0, np.fmax(p1, p2)) < centre - radius)

    axes = [_cross3(v, w), _cross3(w, u), _cross3(u, v), (T[3], T[7], T[11])] + [_cross3(a, e) for a in (u, v, w) for e in edges]
    ok = ~separates(axes[0])
    for L in axes[1:]:
        ok = ok & ~separates(L)
    return ok


def obb_pairs(tris: np.ndarray, obbs: np.ndarray) -> np.ndarray:
    """Triangle i against oriented box i ((n, 16) float32 rows or OBB_DTYPE; `first` is not looked at): does the triangle MEET the box -- obb_meets of
    include/hagrid/obb.h, the separating-axis test over 13 axes (the box's three face normals, the stored normal, the nine cross products of a box axis
    with a triangle edge).  This is the pair alone: a query also asks that the triangle meet the box's bounding box (obb_boxes)."""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12); O = _obb_rows(obbs)
    with np.errstate(all="ignore"):
        return _obb_tri([O[:, i] for i in range(16)], [T[:, i] for i in range(12)])


def obb_boxes(obbs: np.ndarray, grid_lo, grid_hi) -> np.ndarray:
    """obb_box of obb.h: (n, 8) float32 box rows -- c -+ ((|u| + |v|) + |w|) per component, grown by eps = 2^-16 of the largest |coordinate| of the grid box
    on every side, `first` kept; an INACTIVE record (a component that is not finite) gets the inactive box min = 1, max = 0.  Not clipped yet."""
    O = _obb_rows(obbs)
    glo = np.asarray(grid_lo, np.float32); ghi = np.asarray(grid_hi, np.float32)
    eps = np.float32(max(np.abs(glo).max(), np.abs(ghi).max())) * np.float32(1.52587890625e-05)
    B = np.zeros((O.shape[0], 8), dtype=np.float32)
    with np.errstate(all="ignore"):
        r = (np.abs(O[:, 4:7]) + np.abs(O[:, 8:11])) + np.abs(O[:, 12:15])
        B[:, 0:3] = (O[:, 0:3] - r) - eps
        B[:, 4:7] = (O[:, 0:3] + r) + eps
    off = ~np.isfinite(O[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]).all(axis=1)
    B[off, 0:3] = np.float32(1.0); B[off, 4:7] = np.float32(0.0)
    B[:, 3] = O[:, 3]
    return B


def overlap_obbs(tris: np.ndarray, obbs: np.ndarray, k: int = 8, query_labels=None, tri_labels=None, grid=None, chunk_pairs: int = 1 << 21) -> dict:
    """The definition of hagrid_overlap_obbs by brute force.  With aabb(box) = obb_boxes, clipped (clip_boxes) to the box of the grid the query runs over
    (`grid` = (min, max), None: grid_box(tris)), S_i = {j >= first_i : the label of box i (>= 0) is no label of triangle j, triangle j has a surface,
    triangle j meets aabb(box_i) (overlap_pairs), obb_pairs(triangle j, box_i)}: "ids" (n, k) int32 = the min(k, |S|) smallest ids ascending, unused slots
    -1; "counts" = min(|S|, k + 1); "sizes" = |S|.  query_labels (n,) and tri_labels (N, 3) int32: both or neither.  Pairs whose bounding intervals miss
    each other are left out before the tests: the triangle / box test says the same of them."""
    assert (query_labels is None) == (tri_labels is None), "query_labels and tri_labels are given together or not at all"
    glo, ghi = grid_box(tris) if grid is None else grid
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12); O = _obb_rows(obbs)
    B = clip_boxes(obb_boxes(O, glo, ghi), glo, ghi)
    n, N = O.shape[0], T.shape[0]
    first = O[:, 3].view(np.int32).astype(np.int64)
    ids = np.full((n, k), -1, dtype=np.int32); sizes = np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        V = tri_vertices(T)
        tmin = np.fmin(V[:, 0], np.fmin(V[:, 1], V[:, 2])); tmax = np.fmax(V[:, 0], np.fmax(V[:, 1], V[:, 2]))
        surface = tris_have_surface(T)
        tid = np.arange(N, dtype=np.int64)[None, :]
        m = max(1, chunk_pairs // max(N, 1))
        for o in range(0, n if N else 0, m):
            b = B[o:o + m]
            active = (b[:, 0:3] <= b[:, 4:7]).all(axis=1)
            near = ~((tmin[None, :, :] > b[:, None, 4:7]) | (tmax[None, :, :] < b[:, None, 0:3])).any(axis=2)      # the bounds check of the triangle / box test
            near &= active[:, None] & surface[None, :] & (tid >= first[o:o + m, None])
            rows, col = np.nonzero(near)                       # by row, then by id ascending
            if query_labels is not None:
                ql = np.asarray(query_labels, np.int32).reshape(-1)[o + rows]
                keep = ~((ql >= 0)[:, None] & (ql[:, None] == np.asarray(tri_labels, np.int32).reshape(-1, 3)[col])).any(axis=1)
                rows, col = rows[keep], col[keep]
            keep = overlap_pairs(T[col], b[rows]) & obb_pairs(T[col], O[o + rows])
            rows, col = rows[keep], col[keep]
            sz = np.bincount(rows, minlength=b.shape[0])
            sizes[o:o + b.shape[0]] = sz
            pos = np.arange(rows.size) - (np.cumsum(sz) - sz)[rows]
            sel = pos < k
            ids[o + rows[sel], pos[sel]] = col[sel]
    return {"ids": ids, "counts": np.minimum(sizes, k + 1).astype(np.int32), "sizes": sizes}


# ---- overlap lists: ALL of S for every region query (hagrid_box_refs, hagrid_tri_refs, hagrid_obb_refs then unique and compact) --------

def _region_lists(T: np.ndarray, B: np.ndarray, first, needs_surface: bool, pair_filter, chunk_pairs: int) -> dict:
    """Every triangle j >= first[i] that meets the clipped box B[i] (overlap_pairs) and passes pair_filter(query rows, triangle ids) -> bool, per query
    ascending by id, in CSR form.  Pairs whose bounding intervals miss each other are left out before the tests: the triangle / box test says the same."""
    n, N = B.shape[0], T.shape[0]
    sizes = np.zeros(n, dtype=np.int64); chunks = []
    with np.errstate(all="ignore"):
        V = tri_vertices(T)
        tmin = np.fmin(V[:, 0], np.fmin(V[:, 1], V[:, 2])); tmax = np.fmax(V[:, 0], np.fmax(V[:, 1], V[:, 2]))
        surface = tris_have_surface(T) if needs_surface else np.ones(N, dtype=bool)
        tid = np.arange(N, dtype=np.int64)[None, :]
        m = max(1, chunk_pairs // max(N, 1))
        for o in range(0, n if N else 0, m):
            b = B[o:o + m]
            active = (b[:, 0:3] <= b[:, 4:7]).all(axis=1)
            near = ~((tmin[None, :, :] > b[:, None, 4:7]) | (tmax[None, :, :] < b[:, None, 0:3])).any(axis=2)      # the bounds check of the triangle / box test
            near &= active[:, None] & surface[None, :] & (tid >= first[o:o + m, None])
            rows, col = np.nonzero(near)                       # by row, then by id ascending
            keep = overlap_pairs(T[col], b[rows])
            rows, col = rows[keep], col[keep]
            keep = pair_filter(o + rows, col)
            rows, col = rows[keep], col[keep]
            sizes[o:o + b.shape[0]] = np.bincount(rows, minlength=b.shape[0])
            chunks.append(col.astype(np.int32))
    offsets = np.zeros(n + 1, dtype=np.int64); np.cumsum(sizes, out=offsets[1:])
    return {"offsets": offsets, "ids": np.concatenate(chunks) if chunks else np.zeros(0, np.int32)}


def box_lists(tris: np.ndarray, boxes: np.ndarray, grid=None, chunk_pairs: int = 1 << 21) -> dict:
    """The definition of the box lists (hagrid_box_refs, then hagrid_unique_lists and hagrid_compact_lists): ALL of the set S that overlap_boxes defines --
    `first`, the clip and overlap_pairs as there -- for every box, ascending by id: "offsets" int64 (n + 1,), "ids" int32 (total,).  What the pages of the
    k-list concatenate to; overlap_boxes' "sizes" are the list lengths, its "ids" the lists' first k."""
    glo, ghi = grid_box(tris) if grid is None else grid
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12); B = clip_boxes(boxes, glo, ghi)
    return _region_lists(T, B, B[:, 3].view(np.int32).astype(np.int64), False, lambda rows, col: np.ones(rows.size, dtype=bool), chunk_pairs)


def contact_lists(tris: np.ndarray, queries: np.ndarray, first=None, query_labels=None, tri_labels=None, grid=None, chunk_pairs: int = 1 << 21) -> dict:
    """The definition of the contact lists (hagrid_tri_refs ...): ALL of the set S that overlap_tris defines -- first, labels, surface, the grown and clipped
    query box, tri_tri_pairs as there -- for every query, ascending by id, in CSR form as box_lists."""
    assert (query_labels is None) == (tri_labels is None), "query_labels and tri_labels are given together or not at all"
    glo, ghi = grid_box(tris) if grid is None else grid
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12); Q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 12)
    B = clip_boxes(query_boxes(Q, glo, ghi), glo, ghi)
    first = np.zeros(Q.shape[0], np.int64) if first is None else np.asarray(first).astype(np.int64)

    def pair(rows, col):
        keep = np.ones(rows.size, dtype=bool)
        if query_labels is not None:
            keep = ~labels_shared(np.asarray(query_labels).reshape(-1, 3)[rows], np.asarray(tri_labels).reshape(-1, 3)[col])
        keep[keep] = tri_tri_pairs(Q[rows[keep]], T[col[keep]])
        return keep
    return _region_lists(T, B, first, True, pair, chunk_pairs)


def obb_lists(tris: np.ndarray, obbs: np.ndarray, query_labels=None, tri_labels=None, grid=None, chunk_pairs: int = 1 << 21) -> dict:
    """The definition of the oriented-box lists (hagrid_obb_refs ...): ALL of the set S that overlap_obbs defines -- `first`, the label, surface, the grown and
    clipped bounding box, obb_pairs as there -- for every box, ascending by id, in CSR form as box_lists."""
    assert (query_labels is None) == (tri_labels is None), "query_labels and tri_labels are given together or not at all"
    glo, ghi = grid_box(tris) if grid is None else grid
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12); O = _obb_rows(obbs)
    B = clip_boxes(obb_boxes(O, glo, ghi), glo, ghi)

    def pair(rows, col):
        keep = np.ones(rows.size, dtype=bool)
        if query_labels is not None:
            ql = np.asarray(query_labels, np.int32).reshape(-1)[rows]
            keep = ~((ql >= 0)[:, None] & (ql[:, None] == np.asarray(tri_labels, np.int32).reshape(-1, 3)[col])).any(axis=1)
        keep[keep] = obb_pairs(T[col[keep]], O[rows[keep]])
        return keep
    return _region_lists(T, B, O[:, 3].view(np.int32).astype(np.int64), True, pair, chunk_pairs)


# ---- crossing queries: the numpy statement of include/hagrid/crossings.h (same operations, same order, same bits) ---------------------------

INSIDE_WINDING = 1
# the default directions of hagrid_points_inside: (3, 1, 2) / sqrt 14, (-2, 4, 3) / sqrt 29, (1, -5, 2) / sqrt 30 -- the float32 literals of crossings.h
CROSSING_DIRS = np.array([[0.80178373, 0.26726124, 0.53452248], [-0.37139068, 0.74278135, 0.55708601], [0.18257419, -0.91287093, 0.36514837]], dtype=np.float32)


def _prodsign(x, y):
    """prodsign of common.h: x with its sign flipped when y is negative"""
    x, y = np.broadcast_arrays(np.asarray(x, np.float32), np.asarray(y, np.float32))
    return (np.ascontiguousarray(x).view(np.uint32) ^ (np.ascontiguousarray(y).view(np.uint32) & np.uint32(0x80000000))).view(np.float32)


def admit_rays(rays: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """admit_ray of ray.h on (n, 8) float32 rows: (the rays with every zero of dir made +0, whether the ray may enter the cell walk)"""
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8).copy()
    d = r[:, 4:7]
    d[d == 0] = np.float32(0.0)
    with np.errstate(all="ignore"):
        fin = np.isfinite(r[:, 0:3]).all(axis=1) & np.isfinite(d).all(axis=1)
        moves = (np.isfinite(np.float32(1.0) / d) & (d != 0)).any(axis=1)
    return r, fin & moves & ~np.isnan(r[:, 3]) & ~np.isnan(r[:, 7])


def _ray_tri(T, org, dirv, tmin, tmax):
    """intersect_prim_ray of prims.h on broadcastable float32 arrays: T = the 12 columns of the Tri records -> (accept, t, sign bit of det)"""
    v0, e1, e2, n = (T[0], T[1], T[2]), (T[4], T[5], T[6]), (T[8], T[9], T[10]), (T[3], T[7], T[11])
    c = _sub3(v0, org)
    r = _cross3(dirv, c)
    det = _dot3(n, dirv)
    abs_det = np.abs(det)
    u = _prodsign(_dot3(r, e2), det)
    v = _prodsign(_dot3(r, e1), det)
    w = abs_det - u - v
    eps = np.float32(1e-9)
    t = _prodsign(_dot3(n, c), det)
    ok = (u >= -eps) & (v >= -eps) & (w >= -eps) & (t >= abs_det * tmin) & (abs_det * tmax > t)
    tt = (t * (np.float32(1.0) / abs_det)).astype(np.float32)
    return ok & ~np.isnan(tt), tt, np.signbit(det)          # (crosses() of crossings.h: a NaN t -- both dot products overflowed -- is refused)


def ray_tri_pairs(tris: np.ndarray, rays: np.ndarray) -> dict:
    """Triangle i against ray i (rays: (n, 8) float32): "accept" (the ray CROSSES the triangle: intersect_prim_ray of prims.h with the ray's own window; an
    inadmissible ray crosses nothing), "t" and "entering" (the sign bit of det = dot(normal, dir)) -- float32, operation for operation of prims.h."""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    R, adm = admit_rays(rays)
    with np.errstate(all="ignore"):
        ok, t, neg = _ray_tri([T[:, i] for i in range(12)], (R[:, 0], R[:, 1], R[:, 2]), (R[:, 4], R[:, 5], R[:, 6]), R[:, 3], R[:, 7])
    return {"accept": ok & adm, "t": t, "entering": neg}


def _sorted_crossings(tris: np.ndarray, rays: np.ndarray, chunk_pairs: int):
    """every ray against every triangle, a chunk of rays at a time: (the admitted rays R, then parallel arrays ray, triangle, t, entering of the accepted pairs
    sorted by ray, then t, then id) -- what ray_crossings condenses and ray_crossing_lists writes out"""
    T = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
    R, adm = admit_rays(rays)
    n, N = R.shape[0], T.shape[0]
    cols = [T[None, :, i] for i in range(12)]
    m = max(1, chunk_pairs // max(N, 1))
    ray_idx, tri_idx, ts, neg = [], [], [], []
    with np.errstate(all="ignore"):
        for o in range(0, n if N else 0, m):
            r = R[o:o + m]
            ok, t, ng = _ray_tri(cols, (r[:, 0:1], r[:, 1:2], r[:, 2:3]), (r[:, 4:5], r[:, 5:6], r[:, 6:7]), r[:, 3:4], r[:, 7:8])
            ok = ok & adm[o:o + m, None]
            rows, col = np.nonzero(ok)
            ray_idx.append(rows + o); tri_idx.append(col); ts.append(t[rows, col]); neg.append(ng[rows, col])
    if not ray_idx:
        return R, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, bool)
    r = np.concatenate(ray_idx); j = np.concatenate(tri_idx); t = np.concatenate(ts); ng = np.concatenate(neg)
    order = np.lexsort((j, t, r))                  # by ray, then t, then id
    return R, r[order], j[order], t[order], ng[order]


def ray_crossings(tris: np.ndarray, rays: np.ndarray, chunk_pairs: int = 1 << 21) -> np.ndarray:
    """The definition of hagrid_count_crossings by brute force: rays (n, 8) float32 -> HIT_DTYPE records.  With the crossings of a ray sorted by (t, id):
    id = their number m, t = the first t (the bits of tmax when m = 0), u = length = the sequential float32 sum of t[2p+1] - t[2p] over the pairs,
    v = the int32 bits of winding = #leaving - #entering.  Every ray against every triangle, a chunk of rays at a time."""
    R, r, _, t, ng = _sorted_crossings(tris, rays, chunk_pairs)
    n = R.shape[0]
    out = np.zeros(n, dtype=HIT_DTYPE)
    out["t"] = R[:, 7]
    winding = np.zeros(n, dtype=np.int32)
    if r.size:
        count = np.bincount(r, minlength=n).astype(np.int32)
        first = np.cumsum(count) - count
        has = count > 0
        out["id"] = count
        out["t"][has] = t[first[has]]
        np.add.at(winding, r, np.where(ng, -1, 1).astype(np.int32))
        length = np.zeros(n, dtype=np.float32)
        with np.errstate(all="ignore"):                 # (inf - inf on rays whose every crossing has t = inf)
            for p in range(int(count.max()) // 2 if r.size else 0):          # pair p of every ray that has one: the sum stays sequential per ray
                sel = np.flatnonzero(count >= 2 * p + 2)
                a = first[sel] + 2 * p
                length[sel] = length[sel] + (t[a + 1] - t[a])
        out["u"] = length
    out["v"] = winding.view(np.float32)
    return out


def ray_crossing_lists(tris: np.ndarray, rays: np.ndarray, chunk_pairs: int = 1 << 21) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition of hagrid_list_crossings by brute force: rays (n, 8) float32 -> (offsets int64 (n + 1,), t float32 (total,), key int32 (total,)).  The
    crossings of ray i, sorted by (t, id), are the entries offsets[i] .. offsets[i+1]: key = id * 2 + entering.  The same sorted pairs ray_crossings condenses."""
    R, r, j, t, ng = _sorted_crossings(tris, rays, chunk_pairs)
    offsets = np.zeros(R.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=R.shape[0]), out=offsets[1:])
    return offsets, t.astype(np.float32), (j * 2 + ng).astype(np.int32)


RAY_MASK_ALL = 0xFFFFFFFF


def takes_part(ray_idx, tri_idx, filters=None, tri_masks=None) -> np.ndarray:
    """ray_filter.h on parallel index arrays: triangle tri_idx[p] TAKES PART for ray ray_idx[p] exactly when (mask & tri_masks[tri]) != 0 and tri != skip.
    filters: None (every ray sees everything) or (n, 2) integers (mask, skip), the mask read as 32 bits; tri_masks: None (all ones) or one mask per triangle."""
    ray_idx = np.asarray(ray_idx, dtype=np.int64); tri_idx = np.asarray(tri_idx, dtype=np.int64)
    if filters is None:
        mask = np.full(ray_idx.shape, RAY_MASK_ALL, dtype=np.int64); skip = np.full(ray_idx.shape, -1, dtype=np.int64)
    else:
        f = np.asarray(filters).reshape(-1, 2).astype(np.int64)
        mask = f[ray_idx, 0] & RAY_MASK_ALL; skip = f[ray_idx, 1]
    tm = np.full(tri_idx.shape, RAY_MASK_ALL, dtype=np.int64) if tri_masks is None else np.asarray(tri_masks).reshape(-1).astype(np.int64)[tri_idx] & RAY_MASK_ALL
    return ((mask & tm) != 0) & (tri_idx != skip)


def filtered_hits(tris: np.ndarray, rays: np.ndarray, k: int, filters=None, tri_masks=None, chunk_pairs: int = 1 << 21) -> tuple[np.ndarray, np.ndarray]:
    """The definition of hagrid_traverse_grid_filtered by brute force: rays (n, 8) float32 -> (ids int32 (n, k), t float32 (n, k)).  Of the sorted (ray,
    triangle, t) pairs every ray crosses (_sorted_crossings: intersect_prim_ray with the ray's own window, by ray, then t, then id) those whose triangle takes
    part for the ray (takes_part) are the candidates; ray i gets its first min(k, m), unused slots id -1 and the bits of its tmax.  Without filters these are
    the lists of hagrid_traverse_grid_multi."""
    R, r, j, t, _ = _sorted_crossings(tris, rays, chunk_pairs)
    n = R.shape[0]
    keep = takes_part(r, j, filters, tri_masks)
    r, j, t = r[keep], j[keep], t[keep]
    ids = np.full((n, k), -1, dtype=np.int32)
    out_t = np.repeat(np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)[:, 7:8], k, axis=1)
    if r.size:
        first = np.searchsorted(r, np.arange(n))
        slot = np.arange(r.size) - first[r]
        sel = slot < k
        ids[r[sel], slot[sel]] = j[sel]
        out_t[r[sel], slot[sel]] = t[sel]
    return ids, out_t


def crossing_slots(offsets_or_stride, capacity: int, lists, tmax) -> dict:
    """What hagrid_list_crossings leaves in every one of `capacity` slots.  offsets_or_stride: int64 (n + 1,) offsets (the CSR form) or an int S >= 1 (the
    stride form: ray i owns [i * S, (i + 1) * S)); lists: (offsets, t, key) of ray_crossing_lists; tmax (n,) float32.  The room of ray i is 0 when its pair
    of offsets is negative, decreasing or beyond the capacity; its first min(m, room) entries go to its first slots and every slot left over gets the empty
    entry (the bits of tmax, -1).  Returns "t" uint32 bits, "key" int32 and "written" bool (capacity,), "count" = entries written and "short" = rays with m > room."""
    lo, lt, lk = lists
    tb = np.ascontiguousarray(tmax, dtype=np.float32).view(np.uint32)
    n = tb.size
    if np.ndim(offsets_or_stride) == 0:
        first = np.arange(n, dtype=np.int64) * int(offsets_or_stride); room = np.full(n, int(offsets_or_stride), dtype=np.int64)
    else:
        o = np.asarray(offsets_or_stride, dtype=np.int64)
        first = o[:-1].copy(); room = o[1:] - o[:-1]
        room[(first < 0) | (room < 0) | (o[1:] > capacity)] = 0
    out = {"t": np.zeros(capacity, np.uint32), "key": np.zeros(capacity, np.int32), "written": np.zeros(capacity, bool), "count": 0, "short": 0}
    ltb = np.ascontiguousarray(lt, dtype=np.float32).view(np.uint32)
    for i in np.flatnonzero(room > 0):
        m = int(lo[i + 1] - lo[i]); k = min(m, int(room[i])); a = int(first[i])
        assert not out["written"][a:a + room[i]].any(), "two rays own a slot"
        out["t"][a:a + k] = ltb[lo[i]:lo[i] + k]; out["key"][a:a + k] = lk[lo[i]:lo[i] + k]
        out["t"][a + k:a + room[i]] = tb[i]; out["key"][a + k:a + room[i]] = -1
        out["written"][a:a + room[i]] = True
    m_all = (lo[1:] - lo[:-1])
    out["count"] = int(np.minimum(m_all, room).sum()); out["short"] = int((m_all > room).sum())
    return out


def points_inside(tris: np.ndarray, points: np.ndarray, dirs=None, winding: bool = False, chunk_pairs: int = 1 << 21) -> dict:
    """The definition of hagrid_points_inside by brute force: points (n, 4) float32 x, y, z, reach (or POINT_QUERY_DTYPE); dirs: None = CROSSING_DIRS, or
    (1 | 3, 3) float32.  "records" (n, m) HIT_DTYPE: ray_crossings of org = p, tmin = 0, dir = d, tmax = reach, direction fastest; "inside" (n,) int32: 1 when
    2 * votes > m with the vote count & 1 (winding: winding != 0), else 0; -1 for an inactive point (reach < 0 or NaN, a NaN or infinite coordinate), whose
    records are empty (count 0, t = the bits of reach)."""
    P = np.ascontiguousarray(points).view(np.float32).reshape(-1, 4)
    D = CROSSING_DIRS if dirs is None else np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    n, m = P.shape[0], D.shape[0]
    with np.errstate(all="ignore"):
        active = np.isfinite(P[:, 0:3]).all(axis=1) & (P[:, 3] >= np.float32(0.0))
    rays = np.zeros((n, m, 8), dtype=np.float32)
    rays[:, :, 0:3] = P[:, None, 0:3]; rays[:, :, 4:7] = D[None, :, :]; rays[:, :, 7] = P[:, None, 3]
    rec = np.zeros((n, m), dtype=HIT_DTYPE)
    rec["t"] = P[:, None, 3]
    idx = np.flatnonzero(active)
    if idx.size:
        rec[idx] = ray_crossings(tris, rays[idx].reshape(-1, 8), chunk_pairs).reshape(idx.size, m)
    votes = ((rec["v"].view(np.int32) != 0) if winding else (rec["id"] & 1) != 0).sum(axis=1)
    inside = np.where(active, (2 * votes > m).astype(np.int32), np.int32(-1)).astype(np.int32)
    return {"inside": inside, "records": rec}


def lattice_centres(origin, size, n) -> np.ndarray:
    """The points of hagrid_inside_lattice as POINT_QUERY_DTYPE records, x fastest: the centre of voxel c of an axis is origin + (float(c) + 0.5) * size
    in float32; reach +inf."""
    origin = np.asarray(origin, np.float32); size = np.asarray(size, np.float32)
    nx, ny, nz = (int(v) for v in n)
    out = np.zeros(nx * ny * nz, dtype=POINT_QUERY_DTYPE)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for a, c in enumerate((x.reshape(-1), y.reshape(-1), z.reshape(-1))):
        out["p"][:, a] = origin[a] + (c.astype(np.float32) + np.float32(0.5)) * size[a]
    out["r"] = np.float32(np.inf)
    return out


def distance_lattice(tris: np.ndarray, origin, size, n, band: float, chunk_pairs: int = 1 << 21) -> np.ndarray:
    """The definition of hagrid_distance_lattice: closest_points over lattice_centres with r = band (finite, >= 0) -> CLOSEST_DTYPE records, x fastest."""
    pts = lattice_centres(origin, size, n)
    pts["r"] = np.float32(band)
    return closest_points(tris, pts, chunk_pairs)


def lattice_row_rays(origin, size, n, axis: int) -> np.ndarray:
    """The row rays of hagrid_fill_lattice along `axis` (0, 1, 2) as (rows, 8) float32, the lower remaining axis fastest: org = the centre of the row's voxel 0
    (origin + (float(c) + 0.5) * size on all three axes), dir = +e_axis, tmin = -inf, tmax = +inf."""
    origin = np.asarray(origin, np.float32); size = np.asarray(size, np.float32)
    dims = [int(v) for v in n]
    lo, hi = [a for a in range(3) if a != axis]
    slow, fast = np.meshgrid(np.arange(dims[hi]), np.arange(dims[lo]), indexing="ij")
    c = [None, None, None]
    c[axis] = np.zeros(fast.size, np.int64); c[lo] = fast.reshape(-1); c[hi] = slow.reshape(-1)
    rays = np.zeros((fast.size, 8), dtype=np.float32)
    for a in range(3):
        rays[:, a] = origin[a] + (c[a].astype(np.float32) + np.float32(0.5)) * size[a]
    rays[:, 3] = -np.inf; rays[:, 4 + axis] = 1.0; rays[:, 7] = np.inf
    return rays


def fill_lattice(tris: np.ndarray, origin, size, n, axes: int = 7, winding: bool = False, chunk_pairs: int = 1 << 21) -> dict:
    """The definition of hagrid_fill_lattice by brute force (include/hagrid/crossings.h, "the fill"): one ray per voxel ROW of every requested axis (mask: 1 = x,
    2 = y, 4 = z; 0 means 7), lattice_row_rays.  Voxel c of a row lies at tc(c) = centre(c) - centre(0) in float32; the state before c is taken over the
    crossings with t < tc(c) -- searchsorted(t, tc, "left") of ray_crossing_lists: that count & 1, with winding (#leaving - #entering) != 0 --, the final state
    over all of them.  A row whose final state is 1 abstains; otherwise it votes its state.  Returns "inside" int32 (nx * ny * nz,), x fastest: -1 when no row
    through the voxel was usable, else 2 * votes > valid; "records" HIT_DTYPE, the records of the row rays (ray_crossings), axis after axis, and "abstained"
    bool per row in the same order."""
    origin = np.asarray(origin, np.float32); size = np.asarray(size, np.float32)
    nx, ny, nz = (int(v) for v in n)
    axes = int(axes) or 7
    dims = (nx, ny, nz)
    strides = (1, nx, nx * ny)
    valid = np.zeros(nx * ny * nz, np.int32); votes = np.zeros(nx * ny * nz, np.int32)
    records, abstained = [], []
    for a in range(3):
        if not axes & (1 << a):
            continue
        rays = lattice_row_rays(origin, size, n, a)
        records.append(ray_crossings(tris, rays, chunk_pairs))
        o, t, key = ray_crossing_lists(tris, rays, chunk_pairs)
        c = np.arange(dims[a])
        with np.errstate(all="ignore"):
            centre = origin[a] + (c.astype(np.float32) + np.float32(0.5)) * size[a]
            tc = (centre - centre[0]).astype(np.float32)
        lo, hi = [b for b in range(3) if b != a]
        out = np.zeros(rays.shape[0], bool)
        for r in range(rays.shape[0]):
            tr = t[o[r]:o[r + 1]]
            if winding:
                run = np.concatenate([[0], np.cumsum(np.where(key[o[r]:o[r + 1]] & 1, -1, 1))])
                state = run != 0
            else:
                state = (np.arange(tr.size + 1) & 1) != 0
            out[r] = state[-1]
            if out[r]:
                continue
            k = np.searchsorted(tr, tc, "left")
            e = (r % dims[lo]) * strides[lo] + (r // dims[lo]) * strides[hi] + c * strides[a]
            valid[e] += 1
            votes[e] += state[k]
        abstained.append(out)
    inside = np.where(valid == 0, -1, (2 * votes > valid).astype(np.int32)).astype(np.int32)
    return {"inside": inside, "records": np.concatenate(records), "abstained": np.concatenate(abstained)}


def generate_parallel(gen, first: int, count: int, chunk: int = 1 << 20, threads: int | None = None) -> np.ndarray:
    """gen(first, count) -> (count, 8) float32 for any slice (the generators above are counter-based): builds
    [first, first + count) from chunks made on a thread pool (numpy releases the GIL inside its loops)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    out = np.empty((count, 8), dtype=np.float32)
    starts = list(range(0, count, chunk))

    def work(o):
        c = min(chunk, count - o)
        out[o:o + c] = gen(first + o, c)

    with ThreadPoolExecutor(max_workers=threads or min(32, os.cpu_count() or 1)) as ex:
        list(ex.map(work, starts))
    return out


def shard_range(num_items: int, rank: int, world: int) -> tuple[int, int]:
    """Contiguous ray range of rank ``rank``: [g*n/G, (g+1)*n/G)."""
    return (num_items * rank) // world, (num_items * (rank + 1)) // world
