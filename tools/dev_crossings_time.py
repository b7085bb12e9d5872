"""DEV TOOL: what crossing queries cost (hagrid_count_crossings, hagrid_amd/csrc/crossings.hip) -- soup-1M and the stadium mesh with 1024 x 1024 primary
rays, in ONE process, the two launches alternating after a warm-up, every launch between its own pair of events on the context's stream:

  multi_8     hagrid_traverse_grid_multi with k = 8: the same walk, the same triangle tests, 128 bytes stored per ray -- what a caller had before
  crossings   hagrid_count_crossings: one 16-byte record per ray, pages of eight flushed into it; its batch totals (cells, tests, flushes per ray)

  fill        hagrid_list_crossings alone, in CSR form with offsets made beforehand from the counts: the count's walk plus one 8-byte store per crossing
  protocol    api.crossing_lists: count + torch.cumsum + the total to the host + fill, wall clock around the whole call (it waits for the total)

THE EXPECTATION FOR THE LISTS, stated before any run: fill ~ count plus the stores of 8 bytes per crossing -- the walk, the tests and the flushes are the
count's (the six counters per ray say so), and crossings * 8 bytes at the streaming rate of the part is small against the walk.  "Held" is recorded as
median(fill) <= median(crossings) + crossings * 8 bytes / 2 TB/s + the spread of the count launch (p90 - median).

THE BAR FOR THE COUNT LAUNCH: the sink must cost the count path nothing.  --parent FILE names the JSON this tool wrote at the PARENT commit
(its own build, its own process; its "crossings" events are the count launch); the bar is median(crossings) here <= median(crossings) there + the
parent's own spread (p90 - median) in that run, per scene, recorded as "count_no_slower_than_parent".  --no-lists leaves fill and protocol out, so that the
count launch alternates with exactly what it alternates with at the parent commit.

THE EXPECTATION FOR THE COUNT, stated before any run: on the soup the crossing launch is no slower than the k = 8 launch -- it stores 16 bytes per ray where the other
stores 128 and does the same tests (more where a ray has more than eight crossings: it goes on where k = 8 stops).  The margin is the spread of the k = 8
launch in that run (p90 - median).  The tool records whether it held ("expectation_held"); nothing is tuned toward it, and the page capacity of the kernel
was chosen by register count, not by this tool.  Written to --out (default profiles/crossings_time.json) with build.source_hash().

usage: python tools/dev_crossings_time.py [--size 1024] [--launches 40] [--warmup 10] [--scenes soup,stadium] [--parent FILE] [--no-lists] [--out profiles/crossings_time.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
W = int(arg("--size", "1024")); launches = max(20, int(arg("--launches", "40"))); warmup = int(arg("--warmup", "10"))
scenes = arg("--scenes", "soup,stadium").split(",")
out_path = arg("--out", os.path.join(ROOT, "profiles", "crossings_time.json"))
parent = json.load(open(arg("--parent", ""))) if arg("--parent", "") else None
has_lists = hasattr(api, "list_crossings") and "--no-lists" not in sys.argv          # (the same file runs at the parent commit, which has the count only)

mem = api.MemManager(keep=True)
n = W * W
result = {"tool": "tools/dev_crossings_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "rays": n, "launches": launches, "warmup": warmup,
          "expectation": "soup: median(crossings) <= median(multi_8) + (p90(multi_8) - median(multi_8))",
          "expectation_lists": "median(fill) <= median(crossings) + crossings * 8 bytes / 2 TB/s + (p90(crossings) - median(crossings))",
          "bar_count": "median(crossings) <= parent median(crossings) + (parent p90 - parent median), two builds in two processes",
          "parent_source_hash": parent["source_hash"] if parent else None, "scenes": {}}


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 5), "mean_ms": round(float(a.mean()), 5), "min_ms": round(float(a[0]), 5), "p90_ms": round(float(a[int(0.9 * (a.size - 1))]), 5)}


for name in scenes:
    tris = scene.make_soup(1000000) if name == "soup" else scene.make_stadium(1.0)
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, tris.shape[0])
    cam = scene.camera(grid.bbox_min, grid.bbox_max)
    d_rays = mem.alloc(32 * n); d_hits = mem.alloc(16 * n * 8); d_rec = mem.alloc(16 * n); d_tot = mem.alloc(32)
    api.gen_primary_rays(mem, cam, float(cam[4]), W, W, d_rays)
    variants = [("multi_8", lambda: api.traverse_grid_multi(grid, d_tris, d_rays, d_hits, n, 8)), ("crossings", lambda: api.count_crossings(grid, d_tris, d_rays, d_rec, n))]
    d_off = d_ent = d_tot6 = 0
    if has_lists:
        api.count_crossings(grid, d_tris, d_rays, d_rec, n); mem.synchronize()
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(mem.download(d_rec, api.HIT_DTYPE, n)["id"], out=offsets[1:])
        total = int(offsets[-1])
        d_off = mem.upload(offsets); d_ent = mem.alloc(8 * max(total, 1)); d_tot6 = mem.alloc(48)
        variants.append(("fill", lambda: api.list_crossings(grid, d_tris, d_rays, n, d_ent, total, offsets=d_off)))
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    mem.synchronize()
    ms = {k: [] for k, _ in variants}
    for _ in range(launches):
        for k, fn in variants:                             # alternating: one launch of each, in turn
            ms[k].append(api.profile(fn, mem))
    mem.zero(d_tot, 32)
    api.count_crossings(grid, d_tris, d_rays, d_rec, n, d_tot); mem.synchronize()
    tot = mem.download(d_tot, np.int64, 4)
    counts = mem.download(d_rec, api.HIT_DTYPE, n)["id"]
    ev = {k: stats(v) for k, v in ms.items()}
    margin = ev["multi_8"]["p90_ms"] - ev["multi_8"]["median_ms"]
    lists = {}
    if has_lists:
        import torch
        mem.zero(d_tot6, 48)
        api.list_crossings(grid, d_tris, d_rays, n, d_ent, total, offsets=d_off, counters=d_tot6); mem.synchronize()
        tot6 = mem.download(d_tot6, np.int64, 6)
        mem.use_stream(torch.cuda.current_stream().cuda_stream)
        wall = []
        for i in range(warmup // 2 + launches // 2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = api.crossing_lists(grid, d_tris, d_rays, n)
            torch.cuda.synchronize()
            if i >= warmup // 2:
                wall.append((time.perf_counter() - t0) * 1e3)
        del r
        mem.use_stream(None)
        store_ms = total * 8 / 2e12 * 1e3
        spread = ev["crossings"]["p90_ms"] - ev["crossings"]["median_ms"]
        lists = {"total_crossings": total, "list_counters_per_ray": [round(float(v) / n, 4) for v in tot6], "count_counters_equal": bool((tot6[:4] == tot).all()),
                 "fill_over_count": round(ev["fill"]["median_ms"] / ev["crossings"]["median_ms"], 3), "store_ms_at_2TBs": round(store_ms, 5),
                 "fill_is_count_plus_stores": bool(ev["fill"]["median_ms"] <= ev["crossings"]["median_ms"] + store_ms + spread), "protocol_wall": stats(wall)}
    if parent and name in parent.get("scenes", {}):
        pe = parent["scenes"][name]["events"]["crossings"]
        lists["parent_count"] = pe
        lists["count_no_slower_than_parent"] = bool(ev["crossings"]["median_ms"] <= pe["median_ms"] + (pe["p90_ms"] - pe["median_ms"]))
    row = {"grid": grid.summary(), "events": ev, **lists, "cells_per_ray": round(float(tot[1]) / n, 3), "tests_per_ray": round(float(tot[2]) / n, 3), "flushes_per_ray": round(float(tot[3]) / n, 4),
           "crossings_per_ray_mean": round(float(counts.mean()), 3), "crossings_per_ray_max": int(counts.max()), "rays_with_more_than_8": int((counts > 8).sum()),
           "crossings_over_multi_8": round(ev["crossings"]["median_ms"] / ev["multi_8"]["median_ms"], 3), "margin_ms": round(margin, 5),
           "no_slower_than_multi_8": bool(ev["crossings"]["median_ms"] <= ev["multi_8"]["median_ms"] + margin)}
    result["scenes"][name] = row
    print(json.dumps({name: row}), flush=True)
    for p in (d_rays, d_hits, d_rec, d_tot, d_tris, d_off, d_ent, d_tot6):
        mem.free(p)
    grid.free()

held = result["scenes"].get("soup", {}).get("no_slower_than_multi_8")
result["expectation_held"] = held
result["expectation_lists_held"] = {k: v.get("fill_is_count_plus_stores") for k, v in result["scenes"].items()}
result["bar_count_met"] = {k: v.get("count_no_slower_than_parent") for k, v in result["scenes"].items()}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(f"expectation held: {held}; written to " + os.path.relpath(out_path, ROOT))
mem.close()
