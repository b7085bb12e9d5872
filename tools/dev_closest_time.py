"""DEV TOOL: what nearest-surface queries cost (hagrid_closest_points, hagrid_amd/csrc/closest.hip) -- soup-1M and the stadium mesh (0.95M triangles),
default grid parameters, 2^20 queries of three kinds per scene:

  near     surface samples moved by a Gaussian of 1 % of the box diagonal, r = inf
  uniform  uniform in the box enlarged by 10 %, r = inf
  radius   the same uniform points with r = 2 % of the diagonal

and, in the same run, `nearest`: the nearest-hit launch over the same construction format ("traverse.image" = 0) on 1024 x 1024 primary rays.  ONE process,
the four launches alternating after a warm-up, every launch between its own pair of events on the context's stream and under its own time limit (a launch
that does not come back within --limit seconds ends the process with status 3: nothing else is started on the device).  Per kind one more launch with
counters: cells visited, triangles tested and sub-blocks pruned per query.  Nothing is checked: no time was fixed in advance.  Written to --out (default
profiles/closest_time.json) with build.source_hash().

usage: python tools/dev_closest_time.py [--queries 1048576] [--launches 20] [--warmup 3] [--limit 60] [--scenes soup,stadium] [--out profiles/closest_time.json]"""
import json, os, sys, threading
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
nq = int(arg("--queries", str(1 << 20))); launches = int(arg("--launches", "20")); warmup = int(arg("--warmup", "3")); limit = float(arg("--limit", "60"))
scenes = arg("--scenes", "soup,stadium").split(",")
out_path = arg("--out", os.path.join(ROOT, "profiles", "closest_time.json"))
W = 1024


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
result = {"tool": "tools/dev_closest_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "queries": nq, "launches": launches, "warmup": warmup,
          "rays": W * W, "scenes": {}}
for name in scenes:
    tris = scene.make_soup(1000000) if name == "soup" else scene.make_stadium()
    N = tris.shape[0]
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, N); api.setup_traversal(grid)
    assert mem.image_bytes(grid) == 0
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    pts = {"near": np.empty((nq, 4), np.float32), "uniform": np.empty((nq, 4), np.float32)}
    pts["near"][:, 0:3] = scene.make_points_near_surface(tris, lo, hi, nq, 101); pts["near"][:, 3] = np.inf
    pts["uniform"][:, 0:3] = scene.make_points_uniform(lo, hi, nq, 102); pts["uniform"][:, 3] = np.inf
    pts["radius"] = pts["uniform"].copy(); pts["radius"][:, 3] = np.float32(0.02) * diag
    d_pts = {k: mem.upload(v) for k, v in pts.items()}
    d_res = mem.alloc(32 * nq); d_cnt = mem.alloc(32)
    cam = scene.camera(grid.bbox_min, grid.bbox_max)
    d_rays = mem.alloc(32 * W * W); d_hits = mem.alloc(16 * W * W)
    api.gen_primary_rays(mem, cam, float(cam[4]), W, W, d_rays)
    variants = [("nearest", lambda: api.traverse_grid(grid, d_tris, d_rays, d_hits, W * W))]
    for k in ("near", "uniform", "radius"):
        variants.append((k, lambda k=k: api.closest_points(grid, d_tris, d_pts[k], d_res, nq)))
    for _ in range(warmup):
        for vn, fn in variants:
            limited(lambda: (fn(), mem.synchronize()), f"{name} {vn} (warm-up)")
    ms = {vn: [] for vn, _ in variants}
    for _ in range(launches):
        for vn, fn in variants:                                   # alternating: one launch of each, in turn
            ms[vn].append(limited(lambda: api.profile(fn, mem), f"{name} {vn}"))
    ev = {k: stats(v) for k, v in ms.items()}
    row = {"triangles": int(N), "grid": grid.summary(), "events": ev, "kinds": {}}
    for k in ("near", "uniform", "radius"):
        mem.zero(d_cnt, 32)
        limited(lambda: (api.closest_points(grid, d_tris, d_pts[k], d_res, nq, d_cnt), mem.synchronize()), f"{name} {k} (counters)")
        c = mem.download(d_cnt, np.int64, 4)
        found = int((mem.download(d_res, api.CLOSEST_DTYPE, nq)["id"] >= 0).sum())
        t = ev[k]["median_ms"]
        row["kinds"][k] = {"median_ms": t, "over_nearest": round(t / ev["nearest"]["median_ms"], 2), "Mqueries_per_s": round(nq / t / 1e3, 1), "found": found,
                           "cells_per_query": round(c[1] / nq, 2), "tris_per_query": round(c[2] / nq, 2), "pruned_per_query": round(c[3] / nq, 2),
                           "tris_per_query_over_N": float(c[2] / nq / N), "ns_per_tri_test": round(t * 1e6 / max(int(c[2]), 1), 4)}
    result["scenes"][name] = row
    print(json.dumps({name: row}), flush=True)
    for p in list(d_pts.values()) + [d_res, d_cnt, d_rays, d_hits, d_tris]:
        mem.free(p)
    grid.free()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written to " + os.path.relpath(out_path, ROOT))
mem.close()
