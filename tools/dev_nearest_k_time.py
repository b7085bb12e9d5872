"""DEV TOOL: what neighbour queries cost (hagrid_nearest_tris, nearest_tris_kernel of hagrid_amd/csrc/closest.hip) -- soup-1M and the stadium mesh (0.95M
triangles), default grid parameters, 2^20 queries of two kinds per scene:

  near     surface samples moved by a Gaussian of 1 % of the box diagonal, r = inf
  radius   uniform in the box enlarged by 10 %, r = 2 % of the diagonal

Per kind, in ONE process and alternating after a warm-up: hagrid_closest_points (the untouched kernel: the yardstick of the same run) and
hagrid_nearest_tris at k = 1, 2, 4, 8 (entries only), every launch between its own pair of events on the context's stream and under its own time limit (a
launch that does not come back within --limit seconds ends the process with status 3: nothing else is started on the device).  Per launch kind one more
launch with counters: cells visited, triangles tested, sub-blocks pruned and full lists per query.  For `radius`, api.tris_within (k = 8) end to end on torch
tensors, wall clock around a synchronised call, with the number of triangles listed, the pages it took and whether the lists ended within --max-pages (64:
on the stadium mesh a ball of 2 % of the diagonal around a torus holds thousands of triangles, and paging is quadratic in the length of a list).  k = 1 is reported as a ratio to hagrid_closest_points.  Nothing is
checked: no time was fixed in advance.  Written to --out (default profiles/nearest_k_time.json) with build.source_hash().

usage: python tools/dev_nearest_k_time.py [--queries 1048576] [--launches 15] [--warmup 2] [--limit 60] [--scenes soup,stadium] [--max-pages 64] [--out profiles/nearest_k_time.json]"""
import json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
nq = int(arg("--queries", str(1 << 20))); launches = int(arg("--launches", "15")); warmup = int(arg("--warmup", "2")); limit = float(arg("--limit", "60"))
scenes = arg("--scenes", "soup,stadium").split(","); max_pages = int(arg("--max-pages", "64"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "nearest_k_time.json"))
KS = (1, 2, 4, 8)


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
result = {"tool": "tools/dev_nearest_k_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "queries": nq, "launches": launches, "warmup": warmup,
          "scenes": {}}
for name in scenes:
    tris = scene.make_soup(1000000) if name == "soup" else scene.make_stadium()
    N = tris.shape[0]
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, N)
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    pts = {"near": np.empty((nq, 4), np.float32), "radius": np.empty((nq, 4), np.float32)}
    pts["near"][:, 0:3] = scene.make_points_near_surface(tris, lo, hi, nq, 101); pts["near"][:, 3] = np.inf
    pts["radius"][:, 0:3] = scene.make_points_uniform(lo, hi, nq, 102); pts["radius"][:, 3] = np.float32(0.02) * diag
    d_res = mem.alloc(32 * nq); d_ent = mem.alloc(8 * nq * 8); d_cnt = mem.alloc(40)
    row = {"triangles": int(N), "grid": grid.summary(), "kinds": {}}
    for kind in ("near", "radius"):
        d_pts = mem.upload(pts[kind])
        variants = [("closest_points", lambda c=0: api.closest_points(grid, d_tris, d_pts, d_res, nq, c))]
        for k in KS:
            variants.append((f"k{k}", lambda c=0, k=k: api.nearest_tris(grid, d_tris, d_pts, nq, k, entries=d_ent, counters=c)))
        for _ in range(warmup):
            for vn, fn in variants:
                limited(lambda: (fn(), mem.synchronize()), f"{name} {kind} {vn} (warm-up)")
        ms = {vn: [] for vn, _ in variants}
        for _ in range(launches):
            for vn, fn in variants:                                   # alternating: one launch of each, in turn
                ms[vn].append(limited(lambda: api.profile(fn, mem), f"{name} {kind} {vn}"))
        out = {}
        for vn, fn in variants:
            mem.zero(d_cnt, 40)
            limited(lambda: (fn(d_cnt), mem.synchronize()), f"{name} {kind} {vn} (counters)")
            c = mem.download(d_cnt, np.int64, 5)
            out[vn] = dict(stats(ms[vn]), cells_per_query=round(c[1] / nq, 2), tris_per_query=round(c[2] / nq, 2), pruned_per_query=round(c[3] / nq, 2),
                           full_lists=int(c[4]) if vn != "closest_points" else None)
        base = out["closest_points"]["median_ms"]
        for k in KS:
            out[f"k{k}"]["over_closest_points"] = round(out[f"k{k}"]["median_ms"] / base, 3)
        if kind == "radius":
            import torch
            t_pts = torch.from_numpy(pts[kind]).cuda()
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            walls = []
            for _ in range(3):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                got = limited(lambda: api.tris_within(grid, d_tris, t_pts, k=8, max_pages=max_pages), f"{name} tris_within")
                torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
            mem.use_stream(None)
            out["tris_within_k8"] = {"wall_ms": [round(w, 3) for w in walls], "median_ms": round(float(np.median(walls)), 3), "listed": int(got["offsets"][-1].item()),
                                     "longest": int((got["offsets"][1:] - got["offsets"][:-1]).max().item()), "pages": got["pages"], "complete": got["complete"], "max_pages": max_pages}
            del got, t_pts
        row["kinds"][kind] = out
        mem.free(d_pts)
    result["scenes"][name] = row
    print(json.dumps({name: row}), flush=True)
    for p in (d_res, d_ent, d_cnt, d_tris):
        mem.free(p)
    grid.free()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written to " + os.path.relpath(out_path, ROOT))
mem.close()
