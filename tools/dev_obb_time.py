"""DEV TOOL: what oriented-box queries cost (hagrid_overlap_obbs, obb_tris_kernel of hagrid_amd/csrc/overlap.hip) -- soup-1M and the stadium mesh (0.95M
triangles), default grid parameters.  Per scene:

  small    2^20 rotated boxes with half extents of 0.5 % of the box diagonal, centred on near-surface points: k = 1, k = 8 and ANY, each alternating in the
           same run with hagrid_overlap_boxes over the same records' bounding boxes (scene.obb_boxes) at the same k -- a comparison of COST only: the
           bounding box's answer is not the box's
  planks   --planks (default 1024) thin diagonal planks (half extents 50 %, 2 %, 2 % of the diagonal): k = 8, against the same
  totals   cells visited, pairs offered / tests evaluated and blocks pruned per query, from the batch counters

ONE process, the launches alternating after a warm-up, every launch between its own pair of events on the context's stream and under its own time limit (a
launch that does not come back within --limit seconds ends the process with status 3: nothing else is started on the device).  The expectation, stated
beforehand and recorded with the outcome (nothing is asserted): a small rotated box costs no more than 1.5 times its bounding box at the same k (it offers
fewer triangles to a longer test and asks every block three more questions); a plank costs less than a tenth of its bounding box.

--fold: instead, what the launch folded for this kernel's budget slot costs (blob.hip's validate_arrays, which now also answers grid_max_ref): the median
wall time of hagrid_distance_lattice over a 2 x 2 x 2 lattice with no traversal image (one scan of ref_ids and a read-back per call) and of
hagrid_grid_unpack on a blob packed on the device (one validation launch and two read-backs per call; no file, no copy) on soup-1M, 50 calls each.  Run
the same file in a checkout of the parent commit for the other side.

usage: python tools/dev_obb_time.py [--queries 1048576] [--planks 1024] [--launches 20] [--warmup 3] [--limit 60] [--scenes soup,stadium] [--out profiles/obb_time.json] [--fold]"""
import json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
nq = int(arg("--queries", str(1 << 20))); npl = int(arg("--planks", "1024")); launches = int(arg("--launches", "20")); warmup = int(arg("--warmup", "3"))
limit = float(arg("--limit", "60"))
scenes = arg("--scenes", "soup,stadium").split(",")
out_path = arg("--out", os.path.join(ROOT, "profiles", "obb_time.json"))


def limited(fn, what):
    """fn() under its own time limit"""
    def expired():
        print(f"TIME LIMIT: {what} did not finish within {limit} s", flush=True)
        os._exit(3)
    t = threading.Timer(limit, expired); t.daemon = True; t.start()
    try:
        return fn()
    finally:
        t.cancel()


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 5), "mean_ms": round(float(a.mean()), 5), "min_ms": round(float(a[0]), 5), "p90_ms": round(float(a[int(0.9 * (a.size - 1))]), 5)}


mem = api.MemManager(keep=True)
mem.set_option("traverse.image", 0)

if "--fold" in sys.argv:
    tris = scene.make_soup(1000000)
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, tris.shape[0])
    assert mem.image_bytes(grid) == 0
    lo, hi = scene.tris_bbox(tris)
    d_work = mem.alloc(64); d_ids = mem.alloc(32)
    size = ((hi - lo) / np.float32(64.0)).astype(np.float32)

    def lattice():
        api.distance_lattice(grid, d_tris, lo, size, (2, 2, 2), float(size[0]), d_work, ids=d_ids); mem.synchronize()
    import ctypes as C
    ms_unpack = []

    def unpack():
        """pack (not timed), then hagrid_grid_unpack: the header read back, ONE validation launch and its flag read back; in place, no copy, no file"""
        p = C.c_void_p(); n = C.c_size_t()
        api._check(mem, mem._L.hagrid_grid_pack(mem._ctx, C.byref(grid.pod), C.c_void_p(d_tris), int(tris.shape[0]), C.byref(p), C.byref(n)), "grid_pack")
        mem.synchronize()
        g = api.Grid(); g.mem = mem
        t = C.c_void_p(); nt = C.c_int()
        t0 = time.perf_counter()
        api._check(mem, mem._L.hagrid_grid_unpack(mem._ctx, p, n.value, C.byref(g.pod), C.byref(t), C.byref(nt)), "grid_unpack")
        mem.synchronize()
        ms_unpack.append((time.perf_counter() - t0) * 1e3)
        g.free(); mem.free(t.value)
    res = {"tool": "tools/dev_obb_time.py --fold", "num_refs": grid.num_refs}
    for _ in range(3):
        limited(lattice, "distance_lattice (warm-up)")
    ms = []
    for _ in range(50):
        t0 = time.perf_counter(); limited(lattice, "distance_lattice"); ms.append((time.perf_counter() - t0) * 1e3)
    res["distance_lattice_2x2x2_no_image"] = stats(ms)
    for _ in range(53):
        limited(unpack, "grid_unpack")
    res["grid_unpack"] = stats(ms_unpack[3:])
    print(json.dumps(res), flush=True)
    mem.close()
    sys.exit(0)

result = {"tool": "tools/dev_obb_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "queries": nq, "planks": npl, "launches": launches, "warmup": warmup,
          "expectation": "small: obb <= 1.5 x its bounding box at the same k; planks: obb < 0.1 x its bounding box", "scenes": {}}
ANY = api.OVERLAP_ANY
for name in scenes:
    tris = scene.make_soup(1000000) if name == "soup" else scene.tris_from_mesh(*scene.make_stadium_mesh()[:2])
    N = tris.shape[0]
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, N)
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    R = scene.make_rotations(201, nq)
    h = np.float32(0.005) * diag
    small = scene.make_obbs(scene.make_points_near_surface(tris, lo, hi, nq, 101), R[:, :, 0] * h, R[:, :, 1] * h, R[:, :, 2] * h)
    pl = scene.make_obb_planks(lo, hi, npl, 202)
    d_small = mem.upload(small); d_small_box = mem.upload(scene.obb_boxes(small, grid.bbox_min, grid.bbox_max))
    d_pl = mem.upload(pl); d_pl_box = mem.upload(scene.obb_boxes(pl, grid.bbox_min, grid.bbox_max))
    d_ids = mem.alloc(4 * 8 * max(nq, npl)); d_counts = mem.alloc(4 * max(nq, npl)); d_tot = mem.alloc(32)
    variants = {}
    for kn, k, fl in (("k1", 1, 0), ("k8", 8, 0), ("any", 1, ANY)):
        variants[f"small_obb_{kn}"] = (nq, lambda t=0, k=k, fl=fl: api.overlap_obbs(grid, d_tris, d_small, nq, k, d_ids, d_counts, t, fl))
        variants[f"small_aabb_{kn}"] = (nq, lambda t=0, k=k, fl=fl: api.overlap_boxes(grid, d_tris, d_small_box, nq, k, d_ids, d_counts, t, fl))
    variants["plank_obb_k8"] = (npl, lambda t=0: api.overlap_obbs(grid, d_tris, d_pl, npl, 8, d_ids, d_counts, t))
    variants["plank_aabb_k8"] = (npl, lambda t=0: api.overlap_boxes(grid, d_tris, d_pl_box, npl, 8, d_ids, d_counts, t))
    for _ in range(warmup):
        for vn, (_, fn) in variants.items():
            limited(lambda: (fn(), mem.synchronize()), f"{name} {vn} (warm-up)")
    ms = {vn: [] for vn in variants}
    for _ in range(launches):
        for vn, (_, fn) in variants.items():                       # alternating: one launch of each, in turn
            ms[vn].append(limited(lambda: api.profile(fn, mem), f"{name} {vn}"))
    ev = {k: stats(v) for k, v in ms.items()}
    row = {"triangles": int(N), "grid": grid.summary(), "half_extent": float(h), "events": ev, "kinds": {}, "ratios": {}}
    for vn, (n, fn) in variants.items():
        mem.zero(d_tot, 32)
        limited(lambda: (fn(d_tot), mem.synchronize()), f"{name} {vn} (totals)")
        c = mem.download(d_tot, np.int64, 4)
        cnt = mem.download(d_counts, np.int32, n)
        t = ev[vn]["median_ms"]
        row["kinds"][vn] = {"median_ms": t, "Mqueries_per_s": round(n / t / 1e3, 2), "non_empty": int((cnt > 0).sum()), "cells_per_query": round(c[1] / n, 3),
                            "tests_per_query": round(c[2] / n, 3), "pruned_per_query": round(c[3] / n, 3)}
    for kn in ("k1", "k8", "any"):
        r = ev[f"small_obb_{kn}"]["median_ms"] / ev[f"small_aabb_{kn}"]["median_ms"]
        row["ratios"][f"small_{kn}"] = {"obb_to_aabb": round(r, 4), "holds": bool(r <= 1.5)}
    r = ev["plank_obb_k8"]["median_ms"] / ev["plank_aabb_k8"]["median_ms"]
    row["ratios"]["plank_k8"] = {"obb_to_aabb": round(r, 4), "holds": bool(r < 0.1)}
    result["scenes"][name] = row
    print(json.dumps({name: row}), flush=True)
    for p in (d_small, d_small_box, d_pl, d_pl_box, d_ids, d_counts, d_tot, d_tris):
        mem.free(p)
    grid.free()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written to " + os.path.relpath(out_path, ROOT))
mem.close()
