"""DEV TOOL: what filtered traversal costs (hagrid_traverse_grid_filtered, a mode of the kernel of hagrid_amd/csrc/trav_multi.hip) and what carrying it
costs the unfiltered launch -- the method of tools/dev_multi_hit_time.py: configuration 2's scene (soup-1M, default parameters), 1024 x 1024 primary rays, a
Cell grid and a SmallCell grid, ONE process, the variants alternating launch by launch after a warm-up, every launch between its own pair of events.

  multi_1, multi_8       hagrid_traverse_grid_multi (the unfiltered launch).  The same script runs on the PARENT commit (it then measures these alone, the
                         entry point is missing there): give the files it wrote with --parent, and earlier runs of THIS build with --earlier, so that
                         parent and build alternate run by run.  Expectation: the pooled median of this build is no slower than the parent's by more
                         than the parent's own spread (the interquartile range of its pooled launches).  Recorded, not tuned toward.
  ones_1, ones_8         the filtered launch with all-ones ray masks, no skip and all-ones triangle masks: the price of carrying the filter
  masks_1                filtered k = 1 with the masks of the tests (tests/_filtered.py: seven ray masks in turn, triangle j bit j % 5, none when j % 7 == 3)
  bounce_nearest         hagrid_traverse_grid, "traverse.image" = 0, on the bounce rays of the primary hits (origins lifted by the epsilon of frame.h)
  bounce_any_skip        filtered any-hit on the same rays with skip = the triangle each starts from (api.skip_filters)
The last three are context, no bar.  Written to --out (default profiles/filtered_time.json) with build.source_hash().

usage: python tools/dev_filtered_time.py [--size 1024] [--launches 40] [--warmup 10] [--tris 1000000] [--out FILE] [--parent FILE ...] [--earlier FILE ...]"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def args_after(name):
    out = []
    if name in sys.argv:
        for a in sys.argv[sys.argv.index(name) + 1:]:
            if a.startswith("--"):
                break
            out.append(a)
    return out


W = int(arg("--size", "1024")); launches = max(20, int(arg("--launches", "40"))); warmup = int(arg("--warmup", "10"))
num_tris = int(arg("--tris", "1000000"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "filtered_time.json"))
HAS = hasattr(api, "traverse_grid_filtered")
RAY_MASKS = (0xFFFFFFFF, 0x1B, 0x06, 0x3F, 0, 0x15, 0x80000000)


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, q3 = np.percentile(a, 25), np.percentile(a, 75)
    return {"median_ms": round(float(np.median(a)), 5), "q1_ms": round(float(q1), 5), "q3_ms": round(float(q3), 5), "iqr_ms": round(float(q3 - q1), 5),
            "min_ms": round(float(a[0]), 5), "launches": int(a.size)}


mem = api.MemManager(keep=True)
mem.set_option("traverse.image", 0)                       # the nearest-hit launch walks the construction format, as the multi-hit kernel does
tris = scene.make_soup(num_tris)
d_tris = mem.upload(tris)
n = W * W
result = {"tool": "tools/dev_filtered_time.py", "source_hash": _build.source_hash(), "has_filtered_entry": HAS, "device": mem.device_info(),
          "scene": f"soup-{num_tris}", "rays": n, "launches": launches, "warmup": warmup, "grids": {}}

for label, compress in (("cell", False), ("small_cell", True)):
    grid = api.build_all(mem, d_tris, tris.shape[0], compress=compress)
    api.setup_traversal(grid)
    assert mem.image_bytes(grid) == 0 and bool(grid.small_cells) == compress
    cam = scene.camera(grid.bbox_min, grid.bbox_max)
    d_rays = mem.alloc(32 * n); d_hits = mem.alloc(16 * n * 8)
    api.gen_primary_rays(mem, cam, float(cam[4]), W, W, d_rays)
    variants = [(f"multi_{k}", lambda k=k: api.traverse_grid_multi(grid, d_tris, d_rays, d_hits, n, k)) for k in (1, 8)]
    extra = {}
    if HAS:
        import torch
        i = np.arange(n, dtype=np.int64)
        ones = np.full((n, 2), -1, dtype=np.int32)
        test_f = ones.copy(); test_f[:, 0] = np.asarray(RAY_MASKS, np.int64)[i % 7].astype(np.uint32).view(np.int32)
        j = np.arange(num_tris, dtype=np.int64)
        test_m = np.where(j % 7 == 3, 0, (np.int64(1) << (j % 5)) | np.where(j % 11 == 0, 0x20, 0)).astype(np.uint32)
        d_ones_f = mem.upload(ones); d_ones_m = mem.upload(np.full(num_tris, 0xFFFFFFFF, np.uint32))
        d_test_f = mem.upload(test_f); d_test_m = mem.upload(test_m)
        # bounce rays from the primary hits, and the filters that skip the triangle each starts from
        t_hits = torch.empty((n, 4), dtype=torch.int32, device=f"cuda:{mem.device}")
        d_bounce = mem.alloc(32 * n); d_occ = mem.alloc(16 * n)
        torch.cuda.synchronize()
        api.traverse_grid(grid, d_tris, d_rays, t_hits.data_ptr(), n)
        api.gen_bounce_rays(mem, d_tris, d_rays, t_hits.data_ptr(), n, 7, grid.bbox_min, grid.bbox_max, d_bounce, redraw_misses=False)
        t_skip = api.skip_filters(t_hits, mem=mem)
        mem.synchronize()
        for k in (1, 8):
            variants.append((f"ones_{k}", lambda k=k: api.traverse_grid_filtered(grid, d_tris, d_rays, d_hits, n, k, d_ones_f, d_ones_m)))
        variants.append(("masks_1", lambda: api.traverse_grid_filtered(grid, d_tris, d_rays, d_hits, n, 1, d_test_f, d_test_m)))
        variants.append(("bounce_nearest", lambda: api.traverse_grid(grid, d_tris, d_bounce, d_occ, n)))
        variants.append(("bounce_any_skip", lambda: api.traverse_grid_filtered(grid, d_tris, d_bounce, d_occ, n, 1, t_skip.data_ptr(), 0, api.ANY_HIT)))
        extra["primary_hits"] = int((t_hits[:, 0] >= 0).sum().item())
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    mem.synchronize()
    ms = {name: [] for name, _ in variants}
    for _ in range(launches):
        for name, fn in variants:                          # alternating: one launch of each, in turn
            ms[name].append(api.profile(fn, mem))
    ev = {k: stats(v) for k, v in ms.items()}
    row = {"grid": grid.summary(), "events": ev, "samples_ms": {k: [round(float(x), 5) for x in ms[k]] for k in ("multi_1", "multi_8")}, **extra}
    if HAS:
        # the all-ones launch answers what the unfiltered one answers (checked here once, on the timed inputs)
        api.traverse_grid_multi(grid, d_tris, d_rays, d_hits, n, 8); mem.synchronize()
        a = mem.download(d_hits, np.uint32, 4 * n * 8)
        api.traverse_grid_filtered(grid, d_tris, d_rays, d_hits, n, 8, d_ones_f, d_ones_m); mem.synchronize()
        row["ones_8_equals_multi_8"] = bool((a == mem.download(d_hits, np.uint32, 4 * n * 8)).all())
        for k in (1, 8):
            row[f"ones_{k}_over_multi_{k}"] = round(ev[f"ones_{k}"]["median_ms"] / ev[f"multi_{k}"]["median_ms"], 4)
        row["masks_1_over_multi_1"] = round(ev["masks_1"]["median_ms"] / ev["multi_1"]["median_ms"], 4)
        row["bounce_any_skip_over_bounce_nearest"] = round(ev["bounce_any_skip"]["median_ms"] / ev["bounce_nearest"]["median_ms"], 4)
        for p in (d_ones_f, d_ones_m, d_test_f, d_test_m, d_bounce, d_occ):
            mem.free(p)
    result["grids"][label] = row
    print(json.dumps({label: {k: v for k, v in row.items() if k != "samples_ms"}}), flush=True)
    mem.free(d_rays); mem.free(d_hits); grid.free()

# the unfiltered launch against the parent commit: launches pooled over the runs given, parent and build alternating run by run
parents = [json.load(open(p)) for p in args_after("--parent")]
earlier = [json.load(open(p)) for p in args_after("--earlier")]
if parents:
    cmp = {"parent_source_hashes": sorted({p["source_hash"] for p in parents}), "parent_runs": len(parents), "runs_of_this_build": 1 + len(earlier), "grids": {}}
    ok = True
    for label in result["grids"]:
        cmp["grids"][label] = {}
        for name in ("multi_1", "multi_8"):
            par = [x for p in parents for x in p["grids"][label]["samples_ms"][name]]
            own = [x for p in earlier + [result] for x in p["grids"][label]["samples_ms"][name]]
            sp, so = stats(par), stats(own)
            row = {"parent": sp, "this_build": so, "parent_run_medians_ms": [p["grids"][label]["events"][name]["median_ms"] for p in parents],
                   "this_build_run_medians_ms": [p["grids"][label]["events"][name]["median_ms"] for p in earlier + [result]],
                   "this_over_parent": round(so["median_ms"] / sp["median_ms"], 4),
                   "no_slower_than_parent_beyond_its_spread": bool(so["median_ms"] - sp["median_ms"] <= sp["iqr_ms"])}
            ok = ok and row["no_slower_than_parent_beyond_its_spread"]
            cmp["grids"][label][name] = row
    cmp["expectation_holds"] = ok
    result["unfiltered_against_parent"] = cmp
    print(json.dumps({"unfiltered_against_parent": {g: {k: (v["parent"]["median_ms"], v["this_build"]["median_ms"], v["parent"]["iqr_ms"]) for k, v in r.items()} for g, r in cmp["grids"].items()},
                      "expectation_holds": ok}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written to " + os.path.relpath(out_path, ROOT))
mem.close()
