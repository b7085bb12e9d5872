"""What the deep-grid tests (tests/test_deep_grids_cpu.py, tests/test_deep_grids_gpu.py) share: scenes whose grids are 10 to 16 levels deep, the queries
that reach into their deepest cells, the catalogue with the depth every scene must have, and the construction passes one at a time, so that every
consumer of the construction format is walked after build, merge, flatten, expand and compress -- not only on the finished, shallow grids of the
other test files.  A scene is a few stacks of tiny parallel plates: 72 to 144 triangles, built in milliseconds."""
import numpy as np

from hagrid_amd import scene

import _closest as K
import _crossing_lists as CL
import _crossings as X
import _multi_hit as M
import _overlap as V
import _overlap_tris as T

STAGES = ("build", "merge", "flatten", "expand", "compress")
ALPHA, EXPAND_ITERS = 0.995, 3
NUM_RAYS, NUM_BOXES, NUM_POINTS, NUM_CONTACTS = 1024, 384, 512, 144
BOX_EDGES = np.float32([1e-5, 1e-4, 1e-3, 5e-2])
SEED = 0x64656570                        # "deep"
NESTED_CENTRE = np.float32([0.31, 0.47, 0.62])


def _unit(v):
    return v / np.sqrt((v * v).sum())


def plates(stacks: int, per: int, size: float, gap: float, seed: int) -> np.ndarray:
    """`stacks` stacks of `per` parallel triangles of half-width `size`, `gap` apart along their normal, the stacks anywhere in the unit cube"""
    rng = np.random.default_rng(seed)
    centres = rng.random((stacks, 3)).astype(np.float32) * np.float32(0.9) + np.float32(0.05)
    v = np.empty((stacks, per, 3, 3), dtype=np.float64)
    for s in range(stacks):
        a = _unit(rng.standard_normal(3))
        b = _unit(np.cross(a, rng.standard_normal(3)))
        n = np.cross(a, b)
        for p in range(per):
            o = centres[s].astype(np.float64) + n * gap * p
            v[s, p, 0] = o - size * a - size * b
            v[s, p, 1] = o + size * a - 0.3 * size * b
            v[s, p, 2] = o + 0.2 * size * a + size * b
    v = v.reshape(-1, 3, 3).astype(np.float32)
    return scene.tris_from_vertices(v[:, 0], v[:, 1], v[:, 2])


def nested() -> np.ndarray:
    """a soup of 1500 triangles over the unit cube and three more of 1500, scaled by 0.05, 0.05^2 and 0.05^3 about one point: 6000 triangles whose top-level
    cells differ in depth by five levels"""
    parts = [scene.make_soup(1500, seed=3)]
    for level in (1, 2, 3):
        t = scene.make_soup(1500, seed=3 + level)
        verts = scene.tri_vertices(t).astype(np.float32)
        verts = (NESTED_CENTRE + (verts - NESTED_CENTRE) * np.float32(0.05 ** level)).astype(np.float32)
        parts.append(scene.tris_from_vertices(verts[:, 0], verts[:, 1], verts[:, 2]))
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


# name: plates(stacks, per, size, gap, seed) or None for nested(), (top_density, snd_density), the shift the grid must have, whether compress accepts it
CATALOGUE = {
    "s10":    dict(plates=(12, 12, 2e-4, 4e-5, 4), densities=(0.001, 6e6),    shift=10, compress=True),
    "s12":    dict(plates=(12, 12, 2e-4, 4e-5, 4), densities=(0.001, 1e9),    shift=12, compress=True),
    "s15":    dict(plates=(6, 12, 5e-5, 1e-5, 4),  densities=(0.001, 3e11),   shift=15, compress=False),
    "s16":    dict(plates=(6, 12, 5e-5, 1e-5, 4),  densities=(0.001, 2.4e12), shift=16, compress=False),
    "nested": dict(plates=None,                    densities=(0.12, 2.4),     shift=5,  compress=True),
}
WALKED = ("s10", "s12", "s15", "nested")          # s16 is built, and refused by every consumer


def make_rays(name: str, tris: np.ndarray, count: int = NUM_RAYS) -> np.ndarray:
    """the stack rays of a catalogue scene; `nested`: aimed at the soup and the outermost cluster.  The ray / triangle test of the reference accepts
    barycentrics down to -1e-9 of a determinant that is about the square of the triangle's edge: 2e-5 in the outermost cluster, 5e-8 in the second and
    1e-10 in the innermost, where it therefore accepts every triangle whose plane the ray crosses nearby -- a brute force says nothing about rays
    aimed there (slack_crossings)."""
    return stack_rays(tris[:3000] if name == "nested" else tris, count)


def make_boxes(name: str, tris: np.ndarray) -> np.ndarray:
    """the boxes of a catalogue scene; `nested`: around vertices of the three clusters"""
    return boxes(tris, first=1500 if name == "nested" else 0)


def make_tris(name: str) -> np.ndarray:
    p = CATALOGUE[name]["plates"]
    return nested() if p is None else plates(*p)


def stages_of(name: str) -> tuple:
    """the stages whose grid a consumer can walk: compress only where it is accepted"""
    return STAGES if CATALOGUE[name]["compress"] else STAGES[:-1]


def _normals(tris: np.ndarray) -> np.ndarray:
    n = tris[:, [3, 7, 11]].astype(np.float32)
    return (n / np.sqrt((n * n).sum(axis=1, keepdims=True))).astype(np.float32)


def stack_rays(tris: np.ndarray, count: int = NUM_RAYS, seed: int = SEED + 1) -> np.ndarray:
    """rays through the stacks: each starts 0.3 before a surface sample of a random triangle and runs along that triangle's unit normal, tilted by a
    Gaussian of 0.05 and with a random sign; tmin 0, tmax inf"""
    p, j = scene.make_points_surface(tris, count, seed)
    sign = np.where(scene._uniform_rows(seed + 1, count, 1)[:, 0] < np.float32(0.5), np.float32(-1.0), np.float32(1.0))
    d = ((_normals(tris)[j] + np.float32(0.05) * scene.make_gaussian3(seed + 2, count)) * sign[:, None]).astype(np.float32)
    rays = np.zeros((count, 8), dtype=np.float32)
    rays[:, 0:3] = p - np.float32(0.3) * d
    rays[:, 4:7] = d
    rays[:, 7] = np.float32(np.inf)
    return rays


def boxes(tris: np.ndarray, seed: int = SEED + 10, first: int = 0) -> np.ndarray:
    """384 boxes: 256 around vertices of triangles (from triangle `first` on), 128 around uniform points, edges of 1e-5, 1e-4, 1e-3 and 5e-2 in turn"""
    lo, hi = scene.tris_bbox(tris)
    centres = np.concatenate([V.vertices_of(tris[first:], 256, seed), scene.make_points_uniform(lo, hi, NUM_BOXES - 256, seed + 1)])
    return V.boxes_around(centres, BOX_EDGES[np.arange(NUM_BOXES) % 4])


def points(tris: np.ndarray, seed: int = SEED + 20) -> np.ndarray:
    """512 closest-point queries (x, y, z, r): 128 a hundredth of the diagonal from the surface, 128 a few plate gaps from it, 256 uniform; of every four, two
    have r = inf, one 5 % of the diagonal, one a ten-thousandth of it (which most uniform points find nothing within)"""
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    q = np.empty((NUM_POINTS, 4), dtype=np.float32)
    q[0:128, 0:3] = K.near_surface_points(tris, lo, hi, 128, seed)
    q[128:256, 0:3] = K.near_surface_points(tris, lo, hi, 128, seed + 1, sigma=2e-5)
    q[256:, 0:3] = K.uniform_points(lo, hi, NUM_POINTS - 256, seed + 2)
    q[:, 3] = np.float32(np.inf)
    q[2::4, 3] = np.float32(0.05) * diag
    q[3::4, 3] = np.float32(1e-4) * diag
    return q


def contact_queries(name: str, tris: np.ndarray) -> np.ndarray:
    """contact queries, two per picked triangle (144 triangles, or all of a plates scene that has no more).  First half: the triangle moved by half a plate
    gap along its normal -- it lies between two plates of its stack, touches neither, and its grown box meets both.  Second half: the same triangle with its
    third vertex lifted by three gaps, so that it cuts through the plates above it.  `nested` has no gap: a thousandth of the triangle's longest edge
    stands for it."""
    n = tris.shape[0]
    pick = np.arange(n) if n <= NUM_CONTACTS else (np.arange(NUM_CONTACTS, dtype=np.int64) * n) // NUM_CONTACTS
    t = tris[pick]
    p = CATALOGUE[name]["plates"]
    if p is not None:
        gap = np.full(pick.size, np.float32(p[3]), dtype=np.float32)
    else:
        gap = np.float32(2e-3) * np.sqrt(np.maximum((t[:, 4:7] ** 2).sum(axis=1), (t[:, 8:11] ** 2).sum(axis=1))).astype(np.float32)
    nrm = _normals(t)
    v = scene.tri_vertices(t) + (nrm * (np.float32(0.5) * gap)[:, None])[:, None, :]
    lifted = v.copy()
    lifted[:, 2] += nrm * (np.float32(3.0) * gap)[:, None]
    v = np.concatenate([v, lifted]).astype(np.float32)
    return np.ascontiguousarray(scene.tris_from_vertices(v[:, 0], v[:, 1], v[:, 2]))


def slack_crossings(tris: np.ndarray, rays: np.ndarray, ray_idx, tri_idx) -> np.ndarray:
    """for crossings (ray, triangle) that a brute force accepted: does the ray pass OUTSIDE the triangle in float64?  The reference's test accepts
    unnormalised barycentrics down to -1e-9 whatever the triangle's size; for the plates of s15 (determinant about 6e-9) that is a sixth of the plate.
    Such a crossing lies in a voxel whose cell need not list the triangle, so a walk may miss it: there the brute force is no yardstick."""
    v = scene.tri_vertices(tris[np.asarray(tri_idx)]).astype(np.float64)
    o = rays[np.asarray(ray_idx), 0:3].astype(np.float64); d = rays[np.asarray(ray_idx), 4:7].astype(np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n = np.cross(e1, e2)
    det = (n * d).sum(axis=1)
    c = o - v[:, 0]
    r = np.cross(c, d)
    u = -(r * e2).sum(axis=1) / det
    w = (r * e1).sum(axis=1) / det
    return np.minimum(np.minimum(u, w), 1.0 - u - w) < 0.0


# Where the reference's slack decides (slack_crossings), a walk may answer otherwise than its brute force.  Per scene, of the 1024 stack rays: on how many the
# nearest hit may differ (the issue's 1 %), on how many any ray walk may, how many may carry a slack crossing at all; and the last two for the 1536 rays of
# the inside votes.  Measured on the oracle's grids (the same at every stage but for s15's point rays, 88 after build): s10, s12 nothing differs, 147 slack rays;
# s15 3, 15, 159 and 88, 235; nested 6, 49, 51 and 117, 213; s10 and s12 40 slack point rays.  The bounds leave a tenth of headroom, no more: a mask that grew would hollow the comparison.
LEFT_OUT = {"s10": (0, 0, 160, 0, 44), "s12": (0, 0, 160, 0, 44), "s15": (10, 17, 175, 97, 258), "nested": (10, 54, 56, 129, 234)}


def compared(name: str, differ: np.ndarray, slack: np.ndarray, what: str, points: bool = False, nearest: bool = False) -> np.ndarray:
    """The rays on which a walk is held to its brute force: all but `differ`, those on which the HOST walk over the same grid arrays differs from it.  Every
    such ray must carry a slack crossing, and no more of them may there be than LEFT_OUT allows (none on s10 and s12: bit for bit)."""
    bound = LEFT_OUT[name]
    most = bound[3] if points else (bound[0] if nearest else bound[1])
    stray = differ & ~slack
    assert not stray.any(), f"{what}: {stray.sum()} rays differ from the brute force without a crossing by the slack, first at {np.flatnonzero(stray)[:5]}"
    assert differ.sum() <= most, f"{what}: the host walk differs from the brute force on {differ.sum()} rays, at most {most} may"
    assert slack.sum() <= bound[4 if points else 2], f"{what}: {slack.sum()} rays carry a slack crossing"
    return ~differ


def lists_differ(a: dict, a_offsets, b: dict, b_offsets) -> np.ndarray:
    """(n,) bool: the crossing list of the ray ("t" bits and "key", laid out by the offsets given with each) differs in length or in any entry"""
    ao, bo = np.asarray(a_offsets, np.int64), np.asarray(b_offsets, np.int64)
    bad = np.diff(ao) != np.diff(bo)
    for i in np.flatnonzero(~bad):
        x, y = slice(ao[i], ao[i + 1]), slice(bo[i], bo[i + 1])
        bad[i] = (np.asarray(a["t"][x]).view(np.uint32) != np.asarray(b["t"][y]).view(np.uint32)).any() or (a["key"][x] != b["key"][y]).any()
    return bad


def point_rays(pts: np.ndarray) -> np.ndarray:
    """the rays of the inside votes with the three default directions, direction fastest: from the point, tmin 0, tmax = its reach"""
    n = pts.shape[0]
    rays = np.zeros((n, 3, 8), dtype=np.float32)
    rays[:, :, 0:3] = pts[:, None, 0:3]; rays[:, :, 4:7] = scene.CROSSING_DIRS[None, :, :]; rays[:, :, 7] = pts[:, None, 3]
    return np.ascontiguousarray(rays.reshape(n * 3, 8))


def slack_rays(hosts: dict, tris: np.ndarray, rays: np.ndarray, counts: np.ndarray):
    """(the brute-force crossing lists of the rays, their offsets, (n,) bool: a crossing of the ray was accepted by the reference's slack)"""
    counts = np.asarray(counts, np.int64)
    offsets = np.zeros(counts.size + 1, np.int64); np.cumsum(counts, out=offsets[1:])
    lists = CL.host_lists(hosts["lists"], hosts["dir"], tris, rays, int(offsets[-1]), offsets=offsets)
    owner = np.repeat(np.arange(counts.size), counts)
    slack = np.zeros(counts.size, dtype=bool)
    slack[owner[slack_crossings(tris, rays, owner, lists["key"] >> 1)]] = True
    return lists, offsets, slack


def deep_rays(tris: np.ndarray, count: int = 128) -> np.ndarray:
    """`nested`: stack rays aimed at the second cluster, inside the deepest cells of the voxel map; some go on through the innermost one, where a thousand
    triangles lie on a line.  The brute force decides little there (make_rays); they are for the device against the host walk over the same grid, which
    is bit for bit whatever the reference accepts."""
    return stack_rays(tris[3000:4500], count, seed=SEED + 5)


PROGRAMS = {"closest": K, "overlap": V, "contact": T, "crossings": X, "lists": CL, "multi": M}


def build_hosts(directory, sanitize: bool = False) -> dict:
    """the host programs of the six query families (sanitize: their stand-alone sanitized builds), compiled side by side, and under "dir" the directory
    they exchange files in"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(PROGRAMS)) as pool:
        jobs = {name: pool.submit(mod.build_host, directory, sanitize) for name, mod in PROGRAMS.items()}
        h = {name: job.result() for name, job in jobs.items()}
    h["dir"] = directory
    return h


class Scene:
    pass


_ANSWERS = {}


def brute_answers(hosts: dict, name: str) -> Scene:
    """a catalogue scene, its queries and the brute-force answer of every query family; computed once per process and left unchanged"""
    if name in _ANSWERS:
        return _ANSWERS[name]
    from oracle import oracle as O
    d = hosts["dir"]
    s = Scene()
    s.name = name
    s.tris = make_tris(name)
    s.rays, s.boxes, s.points, s.contacts = make_rays(name, s.tris), make_boxes(name, s.tris), points(s.tris), contact_queries(name, s.tris)
    s.grid_box = scene.grid_box(s.tris)
    s.closest = K.host_brute(hosts["closest"], d, s.tris, s.points)
    s.overlap = {k: V.host_brute(hosts["overlap"], d, s.tris, s.boxes, k, grid=s.grid_box) for k in (1, 8)}
    s.contact = T.host_brute(hosts["contact"], d, s.tris, s.contacts, 8, grid=s.grid_box)
    s.records = X.host_query(hosts["crossings"], d, s.tris, rays=s.rays)["records"][:, 0]
    s.lists, s.offsets, s.slack = slack_rays(hosts, s.tris, s.rays, s.records["id"])
    s.multi = M.lists_by_brute_force(s.tris, s.rays, k=8)
    s.hits = O.brute_force(s.tris, s.rays)
    s.inside = X.host_query(hosts["crossings"], d, s.tris, points=s.points)                     # "records" (n, 3), "inside" (n,)
    _, _, s.point_slack = slack_rays(hosts, s.tris, point_rays(s.points), s.inside["records"]["id"].reshape(-1))
    _ANSWERS[name] = s
    return s


def longest_chain(entries: np.ndarray, dims) -> int:
    """the largest number of inner voxel-map words (log_dim = w & 3 > 0) on a path from a top-level entry to a leaf: a breadth-first walk over `entries`,
    the children of an inner word w are the (2^log_dim)^3 words from w >> 2 on"""
    e = np.asarray(entries, np.uint32)
    front = np.arange(int(dims[0]) * int(dims[1]) * int(dims[2]), dtype=np.int64)
    depth = 0
    while True:
        w = e[front]
        inner = front[(w & 3) != 0]
        if inner.size == 0:
            return depth
        depth += 1
        w = e[inner].astype(np.int64)
        first, width = w >> 2, np.int64(1) << (3 * (w & 3))
        front = np.concatenate([f + np.arange(c) for f, c in zip(first, width)])


class OracleStages:
    """the CPU oracle's construction of a catalogue scene, one pass per stage_grid call; .grid is the oracle.Grid"""

    def __init__(self, name: str, tris: np.ndarray):
        self.tris, self.densities, self.grid = tris, CATALOGUE[name]["densities"], None

    def build(self):
        from oracle import oracle as O
        self.grid = O.Grid.build(self.tris, *self.densities)

    def merge(self): self.grid.merge(ALPHA)
    def flatten(self): self.grid.flatten()
    def expand(self): self.grid.expand(self.tris, EXPAND_ITERS)
    def compress(self): return self.grid.compress()


class DeviceStages:
    """the same on the device (hagrid_amd.api); .grid is the api.Grid"""

    def __init__(self, name: str, api, mem, d_tris: int, num_tris: int):
        self.api, self.mem, self.d_tris, self.num_tris, self.densities, self.grid = api, mem, d_tris, num_tris, CATALOGUE[name]["densities"], None

    def build(self):
        self.grid = self.api.Grid()
        self.api.build_grid(self.mem, self.d_tris, self.num_tris, self.grid, *self.densities)

    def merge(self): self.api.merge_grid(self.mem, self.grid, ALPHA)
    def flatten(self): self.api.flatten_grid(self.mem, self.grid)
    def expand(self): self.api.expand_grid(self.mem, self.grid, self.d_tris, EXPAND_ITERS)
    def compress(self): return self.api.compress_grid(self.mem, self.grid)


def stage_grid(stages, stage: str):
    """runs the pass `stage` (one of STAGES, in that order) on an OracleStages or a DeviceStages; returns the grid, and for compress (grid, accepted)"""
    done = getattr(stages, stage)()
    return (stages.grid, bool(done)) if stage == "compress" else stages.grid
