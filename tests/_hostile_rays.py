"""What the hostile-ray tests (tests/test_hostile_rays_cpu.py, tests/test_hostile_rays_gpu.py) and the fixture generator
(tests/golden/make_golden_hostile.py) share: a seeded catalogue of rays a caller can put into a ray buffer and the project's own generators never
produce ("admissible rays"), the batches that embed it among ordinary rays, and an independently written float64 ray / triangle
evaluation.  Everything is regenerated from counters (hagrid_amd/scene.py uniform01); tests/golden/hostile_rays.npz holds the reference brute force's
id / t of every catalogue ray and a checksum of the ray bits.

Scenes: the pair of tests/_closest.py -- a soup (rays in general position to it: tier 1, bit for bit against the brute force) and the stadium mesh
(shared vertices and edges, axis-aligned walls: tier 2, judged by the float64 evaluation where walk and brute force differ).
Grids: the default construction parameters and the two other settings of test_build_sizes_and_densities (tests/test_build_gpu.py): (0.5, 8.0), the
finest there, and (0.15, 3.0), the coarsest there that is not the default (that test holds none coarser than the default); Cells and SmallCells."""
import os

import numpy as np

from hagrid_amd import scene

import _closest as K
import _host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hostile_rays.npz")
SCENES = K.SCENES
make_tris = K.make_tris
GRID_PARAMS = {"default": {}, "fine": dict(top_density=0.5, snd_density=8.0), "coarse": dict(top_density=0.15, snd_density=3.0)}
SEED = 0x686F7374696C65             # "hostile"
F32 = np.float32
INF = F32(np.inf)
NAN = F32(np.nan)
NZ = F32(-0.0)

# ---- the tolerances of tier 2 (float64 geometry) ---------------------------------------------------------------------------------
# T_UNIT: a deviation in t is counted in units of max(|t|, the t that spans one box diagonal): the size of the numbers the float32 test subtracts.
# T_DEV_MEASURED: the largest deviation of the reference brute force's t from the float64 t of the same triangle over the generic family
# (8192 make_rays_incoherent rays into the stadium mesh, seed SEED + 100: 3.29e-7, rounded up; the soup gives 2.13e-7;
# test_tier2_tolerance_is_the_measured_one measures both again and fails if one is larger).  T_TOL is four times that: the walk tests the same triangle
# with the same arithmetic, so it can add no error of its own; the factor covers rays in less general position than the family measured.
T_DEV_MEASURED = 3.3e-7
T_TOL = 4 * T_DEV_MEASURED
# EDGE_MARGIN (barycentric units): the float32 test accepts u, v, w >= -1e-9 * |det| after ~10 roundings of 6e-8 each in terms of the size of the
# triangle's vertices relative to its edges; the stadium's smallest features are 1e-4 of its vertices' coordinates, so 1e-3 is what float32 leaves
# undecided there.  A reported hit must lie in the triangle grown by it; a hit that must not be missed lies in the triangle shrunk by it.
EDGE_MARGIN = 1e-3
# PLANE_MARGIN (|cos| of the angle between ray and triangle normal): below it the ray runs within 0.06 degrees of the triangle's plane, det is a
# difference of products that cancel to < 1e-3 of their size and t = (n . c) / det is not a number float32 decides.  Such a triangle is coplanar to the
# ray: a reported hit on it is called ambiguous, and it is never one that must not be missed.
PLANE_MARGIN = 1e-3
AMBIGUOUS_CAP = 0.05                # of family (k); no other family may hold an ambiguous ray


bits = _host.bits


def oracle_grid(tris, params: dict, compress: bool):
    from oracle import oracle as O
    return O.Grid.full(tris, compress=compress, **params)


def _u(seed, count, width):
    return scene._uniform_rows(SEED + seed, count, width)


def _pick(u, n):
    """float32 uniforms -> integers 0 .. n - 1"""
    return np.minimum((u.astype(np.float64) * n).astype(np.int64), n - 1)


def voxel_planes(G):
    """(lo, hi, res, plane(axis, k)): the planes of the virtual grid as the walk computes them, float(k) * cell_size + lo in float32"""
    lo = np.asarray(G.bbox_min, F32); hi = np.asarray(G.bbox_max, F32)
    res = (np.array(G.dims, np.int64) << G.shift)
    cs = ((hi - lo) / res.astype(F32)).astype(F32)

    def plane(axis, k):
        return (np.asarray(k).astype(F32) * cs[axis] + lo[axis]).astype(F32)
    return lo, hi, res, plane


def _base(lo, hi, n, seed, enlarge=0.0):
    e = F32(enlarge)
    return scene.make_rays_incoherent(lo - e, hi + e, n, SEED + seed)


def _zeroed(base, zero):
    """families (a) / (b): one component (first half) or two components (second half) of the direction set to `zero`"""
    r = base.copy(); n = r.shape[0]; i = np.arange(n); ax = i % 3
    r[i, 4 + ax] = zero
    two = i >= n // 2
    r[i[two], 4 + (ax[two] + 1) % 3] = zero
    last = 4 + (ax + 2) % 3
    r[i, last] = np.where(r[i, last] == 0, F32(0.5), r[i, last])
    return r


WINDOWS = [(0.0, np.inf), (-1.0, np.inf), (-np.inf, np.inf), (-np.inf, 0.5), (np.inf, np.inf), (0.0, -np.inf), (-np.inf, -np.inf), (0.7, 0.2), (0.3, 0.3),
           (0.0, 0.0), (-2.0, -1.0), (-0.5, 0.25), (0.0, 3.4028234663852886e38), (-3.4028234663852886e38, 3.4028234663852886e38), (1e-30, 1e30), (-0.0, 0.4)]


def _admissible(rays) -> np.ndarray:
    """the contract of DESIGN.md section 2, stated on numpy arrays"""
    r = np.asarray(rays, F32)
    fin = np.isfinite(r[:, 0:3]).all(axis=1) & np.isfinite(r[:, 4:7]).all(axis=1)
    with np.errstate(all="ignore"):
        moves = np.isfinite(F32(1.0) / r[:, 4:7]).any(axis=1)          # a component whose float32 reciprocal is finite: not +-0, not below about 2.94e-39
    return fin & moves & ~np.isnan(r[:, 3]) & ~np.isnan(r[:, 7])


def contract_records(rays, k: int = 1) -> np.ndarray:
    """what an inadmissible ray's slot(s) must hold: id -1, t = the bits of its tmax, u = v = 0; (n * k, 4) uint32"""
    n = rays.shape[0]
    rec = np.zeros((n, k, 4), np.uint32)
    rec[:, :, 0] = 0xFFFFFFFF
    rec[:, :, 1] = bits(rays[:, 7])[:, None]
    return rec.reshape(n * k, 4)


def catalogue(tris, G, hit_t=None, mesh=None):
    """The catalogue of a scene and a grid resolution: (rays (n, 8) float32, family (n,) of single letters).  Families c, d, e and part of j lie on the
    voxel planes of G's virtual resolution; everything else depends on the scene alone.  hit_t: what family (h) aims its windows at -- the brute-force t
    of rays_for_hit_windows(tris), NaN for a miss; None: computed here with the oracle's brute force.  mesh: whether family (k) is added (None: for the
    fixture's mesh scene only)."""
    lo, hi, res, plane = voxel_planes(G)
    diag = scene.bbox_diagonal(lo, hi)
    centre = ((lo + hi) * F32(0.5)).astype(F32)
    out = []

    def add(letter, rays):
        rays = np.ascontiguousarray(rays, F32)
        out.append((letter, rays))

    # (a), (b): one or two zero components, +0 and -0
    base = _base(lo, hi, 384, 1, 0.1)
    add("a", _zeroed(base, F32(0.0)))
    add("b", _zeroed(base, NZ))

    # (c), (d): a zero component (either sign), the origin on a voxel plane of that axis / one ulp off it
    c = _base(lo, hi, 384, 2)
    i = np.arange(c.shape[0]); ax = i % 3
    c[i, 4 + ax] = np.where((i // 3) % 2 == 0, F32(0.0), NZ)
    u = _u(3, c.shape[0], 1)[:, 0]
    for a in range(3):
        m = ax == a
        c[m, a] = plane(a, _pick(u[m], int(res[a]) + 1))
    add("c", c)
    up, dn = c.copy(), c.copy()
    up[i, ax] = np.nextafter(c[i, ax], INF); dn[i, ax] = np.nextafter(c[i, ax], -INF)
    den = np.concatenate([up[0::2], dn[1::2]]); i2 = np.concatenate([i[0::2], i[1::2]])          # ... and the same with a component whose reciprocal overflows
    den[np.arange(den.shape[0]), 4 + ax[i2]] = np.where((i2 // 6) % 2 == 0, F32(1e-45), F32(-1e-45))
    add("d", np.concatenate([up, dn, den]))

    # (e): axis-parallel, the origin on voxel planes of both other axes; the origin's own coordinate inside the box or in front of it
    e = _base(lo, hi, 384, 4)
    i = np.arange(e.shape[0]); ax = i % 3
    u = _u(5, e.shape[0], 2)
    sign = np.where((i // 3) % 2 == 0, F32(1.0), F32(-1.0))
    for a in range(3):
        m = ax == a; b, cc = (a + 1) % 3, (a + 2) % 3
        e[m, 4 + a] = sign[m] * np.where((i[m] // 6) % 2 == 0, F32(1.0), np.abs(e[m, 4 + a]) + F32(0.01))
        e[m, 4 + b] = np.where((i[m] // 12) % 2 == 0, F32(0.0), NZ)
        e[m, 4 + cc] = np.where((i[m] // 24) % 2 == 0, F32(0.0), NZ)
        e[m, b] = plane(b, _pick(u[m, 0], int(res[b]) + 1))
        e[m, cc] = plane(cc, _pick(u[m, 1], int(res[cc]) + 1))
        outside = m & ((i // 48) % 2 == 1)
        e[outside, a] = np.where(sign[outside] > 0, lo[a] - F32(0.25) * diag, hi[a] + F32(0.25) * diag)
    add("e", e)

    # (f): origins on the faces, edges and corners of the box (every combination of lo / hi / inside per axis but the all-inside one), pointing into the
    # box, out of it, and along it (the components of the axes that lie on a face zero, of either sign; at a corner: along one of its edges)
    combos = [(x, y, z) for x in range(3) for y in range(3) for z in range(3) if (x, y, z) != (2, 2, 2)]
    f = _base(lo, hi, len(combos) * 3 * 4, 6)
    for j in range(f.shape[0]):
        combo = combos[j % len(combos)]; kind = (j // len(combos)) % 3; rep = j // (3 * len(combos))
        on = [a for a in range(3) if combo[a] != 2]
        for a in on:
            f[j, a] = lo[a] if combo[a] == 0 else hi[a]
        d = f[j, 4:7].copy()
        d = np.where(d == 0, F32(0.25), d)
        inward = np.sign(centre - f[j, 0:3]).astype(F32); inward = np.where(inward == 0, F32(1.0), inward)
        if kind == 0:
            for a in on: d[a] = abs(d[a]) * inward[a]
        elif kind == 1:
            for a in on: d[a] = -abs(d[a]) * inward[a]
        else:
            zero = F32(0.0) if rep % 2 == 0 else NZ
            keep = on[rep % 3] if len(on) == 3 else None
            for a in on:
                d[a] = abs(d[a]) * inward[a] if a == keep else zero
        f[j, 4:7] = d
    add("f", f)

    # (g): denormal and tiny components (the reciprocal of the first overflows), one (first half) or two (second half) per ray
    g = _base(lo, hi, 384, 7, 0.1)
    tiny = np.array([1e-45, -1e-45, 1e-38, -1e-38, 1e-30, -1e-30], F32)
    i = np.arange(g.shape[0]); ax = i % 3
    g[i, 4 + ax] = tiny[(i // 3) % 6]
    two = i >= g.shape[0] // 2
    g[i[two], 4 + (ax[two] + 1) % 3] = tiny[(i[two] // 18) % 6]
    # (l): directions whose ONLY component with a finite reciprocal is next to the smallest that has one (1 / 2.94e-39 is the largest float), the other two
    # zero of either sign or denormal: the least a direction may be and still be admissible
    g2 = _base(lo, hi, 96, 14, 0.1)
    i = np.arange(g2.shape[0]); ax = i % 3
    least = np.array([2.94e-39, -2.94e-39, 3e-39, -3e-39, 1e-38, -1e-38], F32)
    rest = np.array([0.0, -0.0, 1e-45, -1e-45, 2e-39, -2.9e-39], F32)
    g2[i, 4 + ax] = least[(i // 3) % 6]
    g2[i, 4 + (ax + 1) % 3] = rest[(i // 18) % 6]
    g2[i, 4 + (ax + 2) % 3] = rest[(i // 6) % 6]
    add("g", g)
    add("l", g2)          # (a family of its own: |det| of every triangle underflows for such a direction and the brute force answers t = inf with whichever
                          # triangle came last -- it is not well defined there; these rays are held to termination, the conversion modes and device = oracle)

    # (h): windows.  Every pair of WINDOWS on rays of which most hit; then tmax / tmin exactly at the nearest hit's t and one ulp either side
    h = _base(lo, hi, 16 * len(WINDOWS), 8)
    for j, (t0, t1) in enumerate(WINDOWS):
        h[j::len(WINDOWS), 3] = F32(t0); h[j::len(WINDOWS), 7] = F32(t1)
    aim = rays_for_hit_windows(tris)
    if hit_t is None:
        from oracle import oracle as O
        bf = O.brute_force(tris, aim, nthreads=8)
        hit_t = np.where(bf["id"] >= 0, bf["t"], NAN).astype(F32)
    got = ~np.isnan(hit_t)
    aim, t = aim[got][:64], np.asarray(hit_t, F32)[got][:64]          # (the fixture scenes give 64; a scene of three triangles fewer)
    parts = [h]
    for col in (7, 3):
        for tt in (t, np.nextafter(t, INF), np.nextafter(t, -INF)):
            w = aim.copy(); w[:, col] = tt; parts.append(w)
    add("h", np.concatenate(parts))

    # (i): origins 1e3 .. 1e6 box diagonals away, aimed into the box
    far = _base(lo, hi, 256, 9)
    dist = (F32(10.0) ** (F32(3.0) + F32(3.0) * _u(10, far.shape[0], 1)[:, 0])).astype(F32) * diag
    dn_ = far[:, 4:7] / np.sqrt((far[:, 4:7].astype(np.float64) ** 2).sum(1))[:, None].astype(F32)
    far[:, 0:3] = (far[:, 0:3] - dn_ * dist[:, None]).astype(F32)
    add("i", far)

    # (j): every inadmissible class, one component at a time and all at once; zero directions of every sign pattern at generic origins, voxel corners, box corners
    j0 = _base(lo, hi, 512, 11, 0.1)
    j0[:, 7] = np.array([np.inf, 3.4028234663852886e38, 0.5, -1.0], F32)[np.arange(512) % 4]
    n = 0
    for col in (0, 1, 2, 4, 5, 6):
        for val in (NAN, INF, -INF):
            j0[n:n + 4, col] = val; n += 4
    j0[n:n + 4, 3] = NAN; n += 4
    j0[n:n + 4, 7] = NAN; n += 4
    nan_bits = np.array([0x7FC00123, 0xFFC00000, 0x7F800001, 0xFF800001], np.uint32).view(F32)          # quiet with payload, negative, signalling
    j0[n:n + 4, 7] = nan_bits; n += 4
    j0[n:n + 4, 3] = nan_bits; n += 4
    j0[n:n + 4, 0:3] = NAN; j0[n:n + 4, 4:7] = np.array([[1, 1, 1], [-1, -1, -1], [1, -1, 1], [0, 0, 1]], F32); n += 4       # a NaN origin
    j0[n:n + 4, 4:7] = NAN; n += 4                                                                                           # a NaN direction
    j0[n:n + 4, :] = NAN; n += 4
    j0[n:n + 4, 0:3] = INF; j0[n:n + 4, 4:7] = -INF; n += 4
    j0[n:n + 4, :] = np.array([[np.inf] * 8, [-np.inf] * 8, [np.nan, 0, 0, 0, 0, 0, 0, np.nan], [0, 0, 0, np.nan, np.inf, 0, 0, np.inf]], F32); n += 4
    signs = np.array([[F32(0.0) if (p >> a) & 1 == 0 else NZ for a in range(3)] for p in range(8)], F32)
    j0[n:n + 64, 4:7] = signs[np.arange(64) % 8]; n += 64                                  # zero directions at generic origins
    uz = _u(12, 128, 3)
    for q in range(128):                                                                    # ... at voxel corners
        j0[n + q, 0:3] = [plane(a, _pick(uz[q:q + 1, a], int(res[a]) + 1))[0] for a in range(3)]
    j0[n:n + 128, 4:7] = signs[np.arange(128) % 8]; n += 128
    for q in range(16):                                                                     # ... at the box corners, exactly bbox_min / bbox_max among them
        j0[n + q, 0:3] = [lo[a] if (q >> a) & 1 == 0 else hi[a] for a in range(3)]
    j0[n:n + 16, 4:7] = signs[(np.arange(16) // 8 * 7) % 8]; n += 16
    # directions that are not zero but have no component with a finite reciprocal (all below about 2.94e-39): at generic origins, on voxel corners
    sub = np.array([1e-45, -1e-45, 1e-40, -1e-40, 2e-39, -2e-39, 2.9e-39, -2.9e-39, 0.0, -0.0], F32)
    q = np.arange(96)
    d = np.stack([sub[q % 10], sub[(q // 3 + 8) % 10], sub[(q // 7 + 9) % 10]], axis=1)
    d[(d == 0).all(axis=1), 0] = F32(1e-40)
    d[q % 4 == 1] = np.where(np.arange(3)[None, :] == (q[q % 4 == 1, None] // 4) % 3, d[q % 4 == 1, 0:1], F32(0.0))          # a quarter: one component only
    j0[n:n + 96, 4:7] = d
    uz = _u(15, 48, 3)
    for r_ in range(48):
        j0[n + 48 + r_, 0:3] = [plane(a, _pick(uz[r_:r_ + 1, a], int(res[a]) + 1))[0] for a in range(3)]
    n += 96
    add("j", j0[:n])

    rays = np.concatenate([r for _, r in out])
    fam = np.concatenate([np.full(r.shape[0], l) for l, r in out])
    if tris_is_mesh(tris) if mesh is None else mesh:
        km = mesh_family(tris, lo, hi)
        rays = np.concatenate([rays, km]); fam = np.concatenate([fam, np.full(km.shape[0], "k")])
    adm = _admissible(rays)
    assert (adm == (fam != "j")).all(), "family (j) is exactly the inadmissible part of the catalogue"
    return np.ascontiguousarray(rays, F32), fam


def rays_for_hit_windows(tris):
    lo, hi = scene.tris_bbox(tris)
    return _base(lo, hi, 512, 13)


def tris_is_mesh(tris) -> bool:
    """whether tris is make_tris("mesh")"""
    m = make_tris("mesh")
    return tris.shape == m.shape and bool((bits(tris) == bits(m)).all())


def mesh_family(tris, lo, hi):
    """family (k): rays aimed through vertices and through points on edges (shared by two triangles of the mesh), axis-parallel and oblique, and
    rays that run inside the plane of a triangle.  The last kind is kept to 1 / 32 of the family: the brute force's answer to such a ray is ambiguous
    by construction where the ray meets the triangle (AMBIGUOUS_CAP)."""
    n = 1024
    u = _u(20, n, 6)
    t = tris[_pick(u[:, 0], tris.shape[0])]
    v0 = t[:, 0:3]; v1 = v0 - t[:, 4:7]; v2 = v0 + t[:, 8:11]
    which = _pick(u[:, 1], 3)
    a = np.where((which == 0)[:, None], v0, np.where((which == 1)[:, None], v1, v2)).astype(F32)
    b = np.where((which == 0)[:, None], v1, np.where((which == 1)[:, None], v2, v0)).astype(F32)
    i = np.arange(n)
    kind = i % 4                                                    # 0: vertex axis-parallel, 1: vertex oblique, 2: edge axis-parallel, 3: edge oblique
    s = np.where(kind >= 2, u[:, 2], F32(0.0)).astype(F32)
    s = np.where((kind >= 2) & (i % 8 >= 4), F32(0.5), s)           # half of the edge points: the midpoint
    target = (a + (b - a) * s[:, None]).astype(F32)
    base = _base(lo, hi, n, 21)
    d = base[:, 4:7].copy()
    axis = (i // 4) % 3; sign = np.where((i // 12) % 2 == 0, F32(1.0), F32(-1.0))
    par = (kind % 2) == 0
    zero = np.where((i // 24) % 2 == 0, F32(0.0), NZ)
    for c in range(3):
        d[par, c] = np.where(axis[par] == c, sign[par], zero[par])
    back = (F32(0.05) + F32(0.6) * u[:, 3]).astype(F32)
    dn = d / np.sqrt((d.astype(np.float64) ** 2).sum(1))[:, None].astype(F32)
    rays = base.copy()
    rays[:, 0:3] = (target - dn * back[:, None]).astype(F32)
    rays[par, 0:3] = np.where(np.arange(3)[None, :] == axis[par][:, None], rays[par, 0:3], target[par])          # exactly through the target on both other axes
    rays[:, 4:7] = d
    # inside a triangle's plane: from a point of the plane outside the triangle, along an edge direction, towards it
    m = np.flatnonzero(i % 32 == 31)
    e1 = (v1 - v0)[m]; e2 = (v2 - v0)[m]
    dd = (e1 * u[m, 4:5] + e2 * (F32(1.0) - u[m, 4:5])).astype(F32)
    p = (v0[m] + e1 * F32(0.3) + e2 * F32(0.3)).astype(F32)
    rays[m, 4:7] = dd
    rays[m, 0:3] = (p - dd * (F32(1.5) + u[m, 5:6])).astype(F32)
    rays[:, 3] = 0; rays[:, 7] = scene.FLT_MAX
    return rays


def skew_rays(tris, G):
    """Not part of the catalogue: rays with one component 1e-12 .. 1e-30 of the others, the origin one ulp off a voxel plane of that axis (either side).
    Where the voxel was computed on the far side of the plane the exit parameter is a huge negative number and the other axes' voxel coordinates overflow
    int: the walk is right with the device's saturating conversion and not with the C cast of x86, so these rays are held to the
    oracle in ORC_WALK_DEVICE_F2I mode and to the brute force, and the two conversion modes are not required to agree on them."""
    lo, hi, res, plane = voxel_planes(G)
    r = _base(lo, hi, 768, 16)
    i = np.arange(r.shape[0]); ax = i % 3
    big = np.abs(r[:, 4:7]).max(axis=1)
    scale = np.array([1e-12, 1e-14, 1e-16, 1e-18, 1e-20, 1e-24, 1e-30, 1e-36], F32)[(i // 6) % 8]
    r[i, 4 + ax] = np.where((i // 3) % 2 == 0, F32(1.0), F32(-1.0)) * big * scale
    u = _u(17, r.shape[0], 1)[:, 0]
    for a in range(3):
        m = ax == a
        r[m, a] = plane(a, _pick(u[m], int(res[a]) + 1))
    r[i, ax] = np.where((i // 48) % 2 == 0, np.nextafter(r[i, ax], INF), np.nextafter(r[i, ax], -INF))
    return np.ascontiguousarray(r, F32)


def generic_rays(tris, n=8192):
    """the generic family T_DEV_MEASURED was measured on"""
    lo, hi = scene.tris_bbox(tris)
    return _base(lo, hi, n, 100)


# ---- batches ---------------------------------------------------------------------------------------------------------------------

def embed(cat_rays, lo, hi, seed: int = 0):
    """(batch, pos): the catalogue rays among ordinary make_rays_incoherent rays; batch[pos[i]] is catalogue ray i.  Wavefront 0 (slots 0 .. 63) is all
    hostile, wavefront 1 holds one hostile ray in lane 0, wavefront 2 one in lane 63, the rest sit at seeded slots of a tail about twice their number;
    the length is not a multiple of 64."""
    n = cat_rays.shape[0]
    assert n > 66
    rest = n - 66
    tail = 2 * rest + 37
    total = 192 + tail
    if total % 64 == 0:
        total += 1; tail += 1
    order = np.argsort(_u(30 + seed, tail, 1)[:, 0], kind="stable")[:rest]
    pos = np.concatenate([np.arange(64), [64], [191], 192 + np.sort(order)]).astype(np.int64)
    take = np.argsort(_u(40 + seed, n, 1)[:, 0], kind="stable")          # which catalogue ray goes where: families mixed within wavefronts
    batch = scene.make_rays_incoherent(lo - F32(0.1), hi + F32(0.1), total, SEED + 50 + seed)
    where = np.empty(n, np.int64); where[take] = pos
    batch[where] = cat_rays
    assert total % 64 != 0 and len(set(where.tolist())) == n
    return np.ascontiguousarray(batch, F32), where


# ---- float64, written independently: Moeller-Trumbore on the three vertices --------------------------------------------------------

def hits_f64(tris, rays, ids=None):
    """float64 ray / triangle evaluation.  ids None: every ray against every triangle, arrays (num_rays, num_tris); ids given: ray i against triangle
    ids[i], arrays (num_rays,).  Returns t, the barycentrics (b0, b1, b2) of the point where the ray meets the triangle's plane, and cosn = |cos| of the
    angle between the ray and the plane's normal (0: the ray runs inside the plane; t and the barycentrics are then inf / NaN)."""
    T = np.asarray(tris, np.float64); R = np.asarray(rays, np.float64)
    v0 = T[:, 0:3]; v1 = v0 - T[:, 4:7]; v2 = v0 + T[:, 8:11]
    o = R[:, 0:3]; d = R[:, 4:7]
    if ids is not None:
        v0, v1, v2 = v0[ids], v1[ids], v2[ids]
    else:
        v0, v1, v2 = v0[None, :, :], v1[None, :, :], v2[None, :, :]
        o = o[:, None, :]; d = d[:, None, :]
    e1 = v1 - v0; e2 = v2 - v0
    with np.errstate(all="ignore"):
        p = np.cross(d, e2)
        det = (e1 * p).sum(-1)
        s = o - v0
        b1 = (s * p).sum(-1) / det
        q = np.cross(s, e1)
        b2 = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        nrm = np.cross(e1, e2)
        cosn = np.abs((nrm * d).sum(-1)) / (np.sqrt((nrm * nrm).sum(-1)) * np.sqrt((d * d).sum(-1)))
        b0 = 1.0 - b1 - b2
    return t, (b0, b1, b2), np.nan_to_num(cosn, nan=0.0)


def t_unit(tris, rays):
    """the unit deviations of t are counted in: the t that spans one box diagonal"""
    lo, hi = scene.tris_bbox(tris)
    d = np.asarray(rays, np.float64)[:, 4:7]
    return float(scene.bbox_diagonal(lo, hi)) / np.sqrt((d * d).sum(1))


def judge_f64(tris, rays, hits, chunk=256):
    """Tier 2, for rays with finite org / dir and a direction: per ray
    real      -- condition 1: the record is a miss, or a real intersection of that triangle at that t (inside the triangle grown by EDGE_MARGIN, t within
                 T_TOL units of the float64 t, inside the window);
    ambiguous -- the reported triangle is coplanar to the ray (PLANE_MARGIN): float64 has no t to compare with; left out of both conditions;
    missed    -- condition 2 violated: a triangle the ray clearly hits (inside the triangle shrunk by EDGE_MARGIN, not coplanar, inside the window by
                 T_TOL units) lies nearer than the record's t by more than T_TOL units."""
    rays = np.asarray(rays, F32); n = rays.shape[0]
    unit = t_unit(tris, rays)
    ids = hits["id"].astype(np.int64); tt = hits["t"].astype(np.float64)
    has = ids >= 0
    real = np.ones(n, bool); ambiguous = np.zeros(n, bool)
    if has.any():
        t64, (b0, b1, b2), cosn = hits_f64(tris, rays[has], ids[has])
        amb = cosn < PLANE_MARGIN
        scale = np.maximum(np.abs(t64), unit[has])
        with np.errstate(all="ignore"):
            ok = (np.minimum(b0, np.minimum(b1, b2)) >= -EDGE_MARGIN) & (np.abs(tt[has] - t64) <= T_TOL * scale)
            ok &= (tt[has] >= rays[has, 3].astype(np.float64) - T_TOL * scale) & (tt[has] <= rays[has, 7].astype(np.float64) + T_TOL * scale)
        real[has] = ok | amb; ambiguous[has] = amb
    missed = np.zeros(n, bool)
    for o in range(0, n, chunk):
        r = rays[o:o + chunk]
        t64, (b0, b1, b2), cosn = hits_f64(tris, r)
        u = unit[o:o + chunk, None]
        scale = np.maximum(np.abs(t64), u)
        with np.errstate(all="ignore"):
            clear = (np.minimum(b0, np.minimum(b1, b2)) >= EDGE_MARGIN) & (cosn >= PLANE_MARGIN)
            clear &= (t64 >= r[:, 3:4].astype(np.float64) + T_TOL * scale) & (t64 <= r[:, 7:8].astype(np.float64) - T_TOL * scale)
            nearest = np.where(clear, t64, np.inf).min(axis=1)
        limit = np.where(has[o:o + chunk], tt[o:o + chunk], rays[o:o + chunk, 7].astype(np.float64))
        with np.errstate(all="ignore"):
            missed[o:o + chunk] = nearest < limit - T_TOL * np.maximum(np.abs(nearest), unit[o:o + chunk])
    missed &= ~ambiguous
    return {"real": real, "ambiguous": ambiguous, "missed": missed}


def minimum_multiplicity(tris, rays):
    """per ray: how many triangles float64 finds within T_TOL units of the nearest intersection -- intersections in the triangle grown by EDGE_MARGIN, not
    coplanar, inside the window by the same tolerance; 0 when there is none.  1 means the minimum is unique."""
    rays = np.asarray(rays, F32)
    unit = t_unit(tris, rays)
    t64, (b0, b1, b2), cosn = hits_f64(tris, rays)
    scale = np.maximum(np.abs(t64), unit[:, None])
    with np.errstate(all="ignore"):
        cand = (np.minimum(b0, np.minimum(b1, b2)) >= -EDGE_MARGIN) & (cosn >= PLANE_MARGIN)
        cand &= (t64 >= rays[:, 3:4].astype(np.float64) - T_TOL * scale) & (t64 <= rays[:, 7:8].astype(np.float64) + T_TOL * scale)
        t = np.where(cand, t64, np.inf)
        nearest = t.min(axis=1)
        return (t <= (nearest + T_TOL * np.maximum(np.abs(nearest), unit))[:, None]).sum(axis=1) * np.isfinite(nearest)


# FAR_TOL: family (i).  From 1e3 .. 1e6 diagonals away every operand of the float32 test is of the size of the distance D travelled: c = v0 - org is rounded
# to 2^-24 D per component, each component of cross(dir, c) adds two products and a difference, each dot product three products and two sums: about seven
# roundings of 2^-24 D between the inputs and u, v, w, and as many for t.  The point org + t * dir can therefore lie 8 * 2^-23 D off the triangle within its
# plane -- divided by |cos| of the angle between ray and normal, because u, v, w are measured against det = |n| |dir| cos.
FAR_TOL = 8 * 2.0 ** -23


def judge_far(tris, rays, hits):
    """family (i): how far the reported point org + t * dir (float64) lies from the reported triangle, in units of FAR_TOL * distance travelled / |cos|;
    0 for a miss.  (Whether a surface was passed by cannot be asked: surfaces closer together than that are in no order float32 could state, and the walk
    places its voxels with the same error.)"""
    rays = np.asarray(rays, F32)
    out = np.zeros(rays.shape[0])
    has = hits["id"] >= 0
    if has.any():
        r = rays[has].astype(np.float64); ids = hits["id"][has].astype(np.int64)
        P = r[:, 0:3] + hits["t"][has].astype(np.float64)[:, None] * r[:, 4:7]
        dist = K.distance_f64(tris, P, ids)
        travelled = np.abs(hits["t"][has].astype(np.float64)) * np.sqrt((r[:, 4:7] ** 2).sum(1))
        _, _, cosn = hits_f64(tris, rays[has], ids)
        out[has] = dist * np.maximum(cosn, 1e-300) / (FAR_TOL * travelled)
    return out


# ---- fixture -----------------------------------------------------------------------------------------------------------------------

def fixture_key(name: str, grid: str) -> str:
    return f"{name}_{grid}"


def fixture_hits(fixture, name: str, grid: str, rays) -> np.ndarray:
    """the reference brute force's records of the catalogue of (scene, grid setting); fails if the catalogue is not the one the fixture was made from"""
    from oracle import oracle as O
    k = fixture_key(name, grid)
    assert int(fixture[k + "_ray_sum"]) == int(bits(rays).astype(np.uint64).sum()), f"{k}: the catalogue changed: regenerate tests/golden/hostile_rays.npz"
    h = np.zeros(rays.shape[0], O.HIT_DTYPE)
    h["id"] = fixture[k + "_id"]; h["t"] = fixture[k + "_t"]
    return h
