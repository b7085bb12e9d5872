"""DEV TOOL: what the distance lattice by scatter costs (hagrid_distance_lattice, hagrid_amd/csrc/distance.hip) -- soup-1M and the stadium mesh, lattices of 128^3
and 256^3 voxels over the scene's box + 10 %, bands of 1, 3 and 8 voxel edges, in ONE process, the launches alternating after a warm-up, every variant between its
own pair of events on the context's stream:

  scatter      hagrid_distance_lattice (ids and d2), the traversal image of the grid present: no host round trip
  gather       hagrid_closest_points over the same centres with r = band: what a caller had before, the number to beat
  fill         hagrid_fill_lattice, three axes, winding rule: the sign, so that the whole signed field has one line (scatter + fill)
  outside      hagrid_distance_lattice over the SAME lattice moved far outside the scene: every voxel box is empty, so this is the size pass, the scan, the
               initialisation of the slots and the finish -- everything but the splat
  sizes        hagrid_distance_lattice over ONE voxel far outside the scene: the size pass and the scan alone

so the split between the three modes is sizes (size + scan), outside - sizes (slots initialised + finish) and scatter - outside (splat).  Per launch also: pair
tests per voxel (the voxels of all voxel boxes, by the rule of include/hagrid/distance.h stated in numpy here), the share of tests with d2 <= band^2 (counter 2), tasks,
and what the atomics can cost at most: pairs within the band * 8 bytes against the chip-wide atomic rate of the guide (1.3 TB/s) -- an upper bound, since a key
that is not smaller than the slot's is not sent.  No ratio is fixed in advance; the tool records whether the scatter beat the gather per scene, lattice and band.

With --fold the folded ray generators of frame.hip (one kernel since this change) are timed as well: hagrid_gen_primary_rays and hagrid_gen_bounce_rays over 1024^2
rays, medians and spread, to be compared with the same two lines of a run of this tool's --fold part at the parent commit (the entry points are unchanged).

usage: python tools/dev_distance_time.py [--sizes 128,256] [--bands 1,3,8] [--launches 20] [--warmup 3] [--scenes stadium,soup] [--fold] [--out profiles/distance_time.json]"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
sizes = [int(v) for v in arg("--sizes", "128,256").split(",")]
bands = [float(v) for v in arg("--bands", "1,3,8").split(",")]
launches = max(5, int(arg("--launches", "20"))); warmup = int(arg("--warmup", "3"))
scenes = [s for s in arg("--scenes", "stadium,soup").split(",") if s]
out_path = arg("--out", os.path.join(ROOT, "profiles", "distance_time.json"))
ATOMIC_TBPS = 1.3
TASK_VOXELS = 2048

mem = api.MemManager(keep=True)
has_distance = hasattr(api, "distance_lattice")
result = {"tool": "tools/dev_distance_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "launches": launches, "warmup": warmup,
          "atomic_rate_assumed_TBps": ATOMIC_TBPS, "scenes": {}}


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 5), "mean_ms": round(float(a.mean()), 5), "min_ms": round(float(a[0]), 5), "p90_ms": round(float(a[int(0.9 * (a.size - 1))]), 5)}


def box_voxels(tris, lo, hi, origin, size, n, band):
    """the voxels of every triangle's voxel box: tri_box of include/hagrid/distance.h in numpy (float32, the same operations)"""
    f = np.float32
    T = np.ascontiguousarray(tris, dtype=np.float32)
    m = f(band)
    with np.errstate(all="ignore"):
        for a in range(3):
            far = f(origin[a]) + f(n[a]) * f(size[a])
            m = max(m, abs(f(lo[a])), abs(f(hi[a])), abs(f(origin[a])), abs(far))
        reach = f(band) + f(1.52587890625e-05) * f(m)
        vox = np.ones(T.shape[0], np.int64)
        for a in range(3):
            v0 = T[:, a]; v1 = v0 - T[:, 4 + a]; v2 = v0 + T[:, 8 + a]
            tlo = np.minimum(v0, np.minimum(v1, v2)); thi = np.maximum(v0, np.maximum(v1, v2))
            f0 = ((tlo - reach) - f(origin[a])) / f(size[a]); f1 = ((thi + reach) - f(origin[a])) / f(size[a])
            top = min(f(n[a]) + f(2.0), f(2147483520.0))
            empty = f1 < f(-1.0)
            f0 = np.minimum(np.maximum(f0, f(0.0)), top); f1 = np.minimum(np.maximum(f1, f(0.0)), top)
            c0 = np.maximum(f0.astype(np.int64) - 1, 0)
            c1 = np.where(f1.astype(np.int64) < n[a] - 2, f1.astype(np.int64) + 1, n[a] - 1)
            vox *= np.where(empty | (c1 < c0), 0, c1 - c0 + 1)
    vox[(T[:, 3] == 0) & (T[:, 7] == 0) & (T[:, 11] == 0)] = 0
    return vox


for name in scenes:
    if not has_distance:
        break
    tris = scene.make_soup(1000000) if name == "soup" else scene.make_stadium(1.0)
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, tris.shape[0])
    api.setup_traversal(grid)
    lo, hi = np.asarray(grid.bbox_min, np.float32), np.asarray(grid.bbox_max, np.float32)
    ext = (hi - lo).astype(np.float32)
    result["scenes"][name] = {"triangles": int(tris.shape[0]), "grid": grid.summary(), "lattices": {}}
    for N in sizes:
        n = (N, N, N)
        origin = (lo - np.float32(0.05) * ext).astype(np.float32)
        size = (ext * np.float32(1.1) / np.float32(N)).astype(np.float32)
        away = (origin + np.float32(100.0) * ext).astype(np.float32)
        voxels = N * N * N
        pts = scene.lattice_centres(origin, size, n)
        d_pts = mem.upload(pts); d_res = mem.alloc(32 * voxels)
        d_slots = mem.alloc(8 * voxels); d_ids = mem.alloc(4 * voxels); d_d2 = mem.alloc(4 * voxels)
        d_in = mem.alloc(4 * voxels); d_ws = mem.alloc(voxels); d_tot = mem.alloc(32)
        rows = {}
        for k in bands:
            band = np.float32(k) * size.max()
            pts["r"] = band
            mem.copy_h2d(d_pts, pts)
            variants = [("scatter", lambda: api.distance_lattice(grid, d_tris, origin, size, n, band, d_slots, ids=d_ids, d2=d_d2)),
                        ("gather", lambda: api.closest_points(grid, d_tris, d_pts, d_res, voxels)),
                        ("fill", lambda: api.fill_lattice(grid, d_tris, origin, size, n, d_in, axes=7, workspace=d_ws, flags=api.INSIDE_WINDING)),
                        ("outside", lambda: api.distance_lattice(grid, d_tris, away, size, n, band, d_slots, ids=d_ids, d2=d_d2)),
                        ("sizes", lambda: api.distance_lattice(grid, d_tris, away, size, (1, 1, 1), band, d_slots, ids=d_ids, d2=d_d2))]
            for _ in range(warmup):
                for _, fn in variants:
                    fn()
            mem.synchronize()
            ms = {v: [] for v, _ in variants}
            for _ in range(launches):
                for v, fn in variants:                     # alternating: one launch of each, in turn
                    ms[v].append(api.profile(fn, mem))
            mem.zero(d_tot, 32)
            api.distance_lattice(grid, d_tris, origin, size, n, band, d_slots, ids=d_ids, d2=d_d2, counters=d_tot); mem.synchronize()
            tot = mem.download(d_tot, np.int64, 4)
            # the same answers as the gather, bit for bit
            api.closest_points(grid, d_tris, d_pts, d_res, voxels); mem.synchronize()
            res = mem.download(d_res, scene.CLOSEST_DTYPE, voxels)
            same = bool((mem.download(d_ids, np.int32, voxels) == res["id"]).all() and (mem.download(d_d2, np.uint32, voxels) == res["d2"].view(np.uint32)).all())
            del res
            tests = int(box_voxels(tris, lo, hi, origin, size, n, band).sum())
            ev = {v: stats(t) for v, t in ms.items()}
            med = lambda v: ev[v]["median_ms"]
            row = {"band": float(band), "band_voxels": k, "voxels": voxels, "events": ev, "equal_to_gather": same,
                   "triangles_with_a_box": int(tot[0]), "tasks": int(tot[1]), "pairs_within_band": int(tot[2]), "voxels_found": int(tot[3]),
                   "share_found": round(float(tot[3]) / voxels, 4), "pair_tests": tests, "pair_tests_per_voxel": round(tests / voxels, 3),
                   "share_of_tests_within_band": round(float(tot[2]) / max(tests, 1), 4), "task_fill": round(tests / max(float(tot[1]) * TASK_VOXELS, 1.0), 4),
                   "ns_per_pair_test": round(1e6 * max(med("scatter") - med("outside"), 0.0) / max(tests, 1), 5),
                   "atomic_ms_at_most": round(float(tot[2]) * 8 / (ATOMIC_TBPS * 1e9), 5),
                   "mode_ms": {"size_and_scan": med("sizes"), "init_and_finish": round(med("outside") - med("sizes"), 5), "splat": round(med("scatter") - med("outside"), 5)},
                   "scatter_over_gather": round(med("scatter") / med("gather"), 4), "signed_field_ms": round(med("scatter") + med("fill"), 5),
                   "faster_than_gather": bool(med("scatter") < med("gather"))}
            rows[str(k)] = row
            print(json.dumps({name: {str(N): {str(k): row}}}), flush=True)
        result["scenes"][name]["lattices"][str(N)] = rows
        for p in (d_pts, d_res, d_slots, d_ids, d_d2, d_in, d_ws, d_tot):
            mem.free(p)
    mem.free(d_tris)
    grid.free()

if "--fold" in sys.argv:
    # the two ray generators (one kernel since hagrid_distance_lattice took a slot of the kernel budget): the same lines at the parent commit are the comparison
    tris = scene.make_soup(100000)
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, tris.shape[0])
    api.setup_traversal(grid)
    W = 1024
    cam = scene.camera(grid.bbox_min, grid.bbox_max)
    d_rays = mem.alloc(32 * W * W); d_hits = mem.alloc(16 * W * W); d_out = mem.alloc(32 * W * W)
    api.gen_primary_rays(mem, cam, 0.0, W, W, d_rays)
    api.traverse_grid(grid, d_tris, d_rays, d_hits, W * W)
    variants = [("gen_primary_rays", lambda: api.gen_primary_rays(mem, cam, 0.0, W, W, d_rays)),
                ("gen_bounce_rays", lambda: api.gen_bounce_rays(mem, d_tris, d_rays, d_hits, W * W, 7, grid.bbox_min, grid.bbox_max, d_out))]
    for _ in range(10):
        for _, fn in variants:
            fn()
    mem.synchronize()
    ms = {v: [] for v, _ in variants}
    for _ in range(200):
        for v, fn in variants:
            ms[v].append(api.profile(fn, mem))
    result["fold"] = {"rays": W * W, "launches": 200, "has_distance_lattice": has_distance, "events": {v: stats(t) for v, t in ms.items()}}
    print(json.dumps({"fold": result["fold"]}), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written to " + os.path.relpath(out_path, ROOT))
mem.close()
