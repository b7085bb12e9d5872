"""DEV TOOL: what multi-hit traversal costs (hagrid_traverse_grid_multi, hagrid_amd/csrc/trav_multi.hip) -- configuration 2's scene (soup-1M, default
parameters) with 1024 x 1024 primary rays, on a Cell grid and on a SmallCell (compressed) grid, in ONE process, the variants alternating launch by launch
after a warm-up, every launch between its own pair of events on the context's stream:

  nearest   hagrid_traverse_grid with "traverse.image" = 0: the nearest-hit walk of the same construction format (traverse_kernel_v2) -- the baseline,
            and the only tool a caller had before: k launches of it (which return wrong lists)
  multi_k   hagrid_traverse_grid_multi with k = 1, 2, 4, 8

One condition is checked, per grid: time(k = 8) < 8 x time(nearest) (the exit status says so).  time(k = 1) / time(nearest) is recorded as the price of
the list code; nothing is tuned toward either figure.  Written to --out (default profiles/multi_hit_time.json) with build.source_hash().

usage: python tools/dev_multi_hit_time.py [--size 1024] [--launches 40] [--warmup 10] [--tris 1000000] [--out profiles/multi_hit_time.json]"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
W = int(arg("--size", "1024")); launches = max(20, int(arg("--launches", "40"))); warmup = int(arg("--warmup", "10"))
num_tris = int(arg("--tris", "1000000"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "multi_hit_time.json"))
KS = (1, 2, 4, 8)

mem = api.MemManager(keep=True)
mem.set_option("traverse.image", 0)                       # the nearest-hit baseline walks the construction format, as the multi-hit kernel does
tris = scene.make_soup(num_tris)
d_tris = mem.upload(tris)
n = W * W
result = {"tool": "tools/dev_multi_hit_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "scene": f"soup-{num_tris}",
          "rays": n, "launches": launches, "warmup": warmup, "grids": {}}


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 5), "mean_ms": round(float(a.mean()), 5), "min_ms": round(float(a[0]), 5), "p90_ms": round(float(a[int(0.9 * (a.size - 1))]), 5)}


ok = True
for label, compress in (("cell", False), ("small_cell", True)):
    grid = api.build_all(mem, d_tris, tris.shape[0], compress=compress)
    api.setup_traversal(grid)
    assert mem.image_bytes(grid) == 0 and bool(grid.small_cells) == compress
    cam = scene.camera(grid.bbox_min, grid.bbox_max)
    d_rays = mem.alloc(32 * n); d_hits = mem.alloc(16 * n * max(KS))
    api.gen_primary_rays(mem, cam, float(cam[4]), W, W, d_rays)
    variants = [("nearest", lambda: api.traverse_grid(grid, d_tris, d_rays, d_hits, n))]
    for k in KS:
        variants.append((f"multi_{k}", lambda k=k: api.traverse_grid_multi(grid, d_tris, d_rays, d_hits, n, k)))
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    mem.synchronize()
    ms = {name: [] for name, _ in variants}
    for _ in range(launches):
        for name, fn in variants:                          # alternating: one launch of each, in turn
            ms[name].append(api.profile(fn, mem))
    # how many slots the k = 8 lists use (the work the launch did)
    api.traverse_grid_multi(grid, d_tris, d_rays, d_hits, n, 8); mem.synchronize()
    used = (mem.download(d_hits, api.HIT_DTYPE, n * 8)["id"].reshape(n, 8) >= 0).sum(axis=1)
    ev = {k: stats(v) for k, v in ms.items()}
    base = ev["nearest"]["median_ms"]
    row = {"grid": grid.summary(), "events": ev, "hits_per_ray_histogram_k8": np.bincount(used, minlength=9).tolist(),
           "k8_over_nearest": round(ev["multi_8"]["median_ms"] / base, 3), "k1_over_nearest": round(ev["multi_1"]["median_ms"] / base, 3),
           "k8_faster_than_8_nearest_launches": bool(ev["multi_8"]["median_ms"] < 8.0 * base)}
    ok = ok and row["k8_faster_than_8_nearest_launches"]
    result["grids"][label] = row
    print(json.dumps({label: row}), flush=True)
    mem.free(d_rays); mem.free(d_hits); grid.free()

result["condition_k8_faster_than_8_nearest_launches"] = ok
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(("OK" if ok else "FAILED") + ": multi-hit k = 8 faster than eight nearest-hit launches; written to " + os.path.relpath(out_path, ROOT))
mem.close()
sys.exit(0 if ok else 1)
