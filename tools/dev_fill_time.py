"""DEV TOOL: what the scan-line fill costs (hagrid_fill_lattice, the row form of hagrid_amd/csrc/crossings.hip) -- the stadium mesh and soup-1M, lattices of
128^3 and 256^3 voxels over the scene's box, in ONE process, the launches alternating after a warm-up, every variant between its own pair of events on the
context's stream:

  fill_xyz     hagrid_fill_lattice, all three axes, winding rule (three launches)
  fill_z       hagrid_fill_lattice, axis z alone, winding rule (one launch, no workspace)
  inside_3     hagrid_inside_lattice over the same lattice with the three default directions: three rays per VOXEL
  inside_1     hagrid_inside_lattice with one direction
  rows_xyz     hagrid_count_crossings over the SAME row rays as fill_xyz (scene.lattice_row_rays, uploaded): the row walks without the voxel stores
  rows_z       the same for the z rows alone

THE EXPECTATION, stated before any run:
  (1) fill_xyz is faster than inside_3 at the same commit: 3 n^2 rays instead of 3 n^3;
  (2) its time is explained by its row walks: median(fill) <= median(rows) + (p90(fill) - median(fill)); what is left beyond that margin is the stores
      (4 bytes of `inside` per voxel and, with three axes, two writes and two reads of a workspace byte).
The ratios fill / inside and fill / rows and whether (1) and (2) held are recorded per scene and lattice; nothing is tuned toward them.  The soup is no solid:
its answers mean nothing, its rows are the long ones.  Written to --out (default profiles/fill_time.json) with build.source_hash().

usage: python tools/dev_fill_time.py [--sizes 128,256] [--launches 20] [--warmup 5] [--scenes stadium,soup] [--out profiles/fill_time.json]"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
sizes = [int(v) for v in arg("--sizes", "128,256").split(",")]
launches = max(10, int(arg("--launches", "20"))); warmup = int(arg("--warmup", "5"))
scenes = arg("--scenes", "stadium,soup").split(",")
out_path = arg("--out", os.path.join(ROOT, "profiles", "fill_time.json"))

mem = api.MemManager(keep=True)
result = {"tool": "tools/dev_fill_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "launches": launches, "warmup": warmup,
          "expectation_1": "median(fill_xyz) < median(inside_3)",
          "expectation_2": "median(fill) <= median(rows) + (p90(fill) - median(fill)), for xyz and for z", "scenes": {}}


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 5), "mean_ms": round(float(a.mean()), 5), "min_ms": round(float(a[0]), 5), "p90_ms": round(float(a[int(0.9 * (a.size - 1))]), 5)}


for name in scenes:
    tris = scene.make_soup(1000000) if name == "soup" else scene.make_stadium(1.0)
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, tris.shape[0])
    lo, hi = np.asarray(grid.bbox_min, np.float32), np.asarray(grid.bbox_max, np.float32)
    result["scenes"][name] = {"grid": grid.summary(), "lattices": {}}
    for N in sizes:
        n = (N, N, N)
        size = ((hi - lo) / np.float32(N)).astype(np.float32)
        voxels = N * N * N
        rays = np.concatenate([scene.lattice_row_rays(lo, size, n, a) for a in range(3)])
        rows = rays.shape[0]
        d_rays = mem.upload(rays); d_rec = mem.alloc(16 * rows)
        d_in = mem.alloc(4 * voxels); d_ws = mem.alloc(voxels); d_tot = mem.alloc(40)
        one_dir = scene.CROSSING_DIRS[:1]
        variants = [("fill_xyz", lambda: api.fill_lattice(grid, d_tris, lo, size, n, d_in, axes=7, workspace=d_ws, flags=api.INSIDE_WINDING)),
                    ("inside_3", lambda: api.inside_lattice(grid, d_tris, lo, size, n, d_in, flags=api.INSIDE_WINDING)),
                    ("rows_xyz", lambda: api.count_crossings(grid, d_tris, d_rays, d_rec, rows)),
                    ("fill_z", lambda: api.fill_lattice(grid, d_tris, lo, size, n, d_in, axes=4, flags=api.INSIDE_WINDING)),
                    ("inside_1", lambda: api.inside_lattice(grid, d_tris, lo, size, n, d_in, dirs=one_dir, flags=api.INSIDE_WINDING)),
                    ("rows_z", lambda: api.count_crossings(grid, d_tris, d_rays + 32 * 2 * N * N, d_rec, N * N))]
        for _ in range(warmup):
            for _, fn in variants:
                fn()
        mem.synchronize()
        ms = {k: [] for k, _ in variants}
        for _ in range(launches):
            for k, fn in variants:                         # alternating: one launch of each, in turn
                ms[k].append(api.profile(fn, mem))
        mem.zero(d_tot, 40)
        api.fill_lattice(grid, d_tris, lo, size, n, d_in, axes=7, workspace=d_ws, counters=d_tot, flags=api.INSIDE_WINDING); mem.synchronize()
        tot = mem.download(d_tot, np.int64, 5)
        ins = mem.download(d_in, np.int32, voxels)
        ev = {k: stats(v) for k, v in ms.items()}
        spread = lambda k: ev[k]["p90_ms"] - ev[k]["median_ms"]
        row = {"voxels": voxels, "rows": rows, "events": ev, "cells_per_row": round(float(tot[1]) / rows, 3), "tests_per_row": round(float(tot[2]) / rows, 3),
               "flushes_per_row": round(float(tot[3]) / rows, 4), "rows_abstained": int(tot[4]), "voxels_inside": int((ins == 1).sum()), "voxels_undecided": int((ins < 0).sum()),
               "fill_xyz_over_inside_3": round(ev["fill_xyz"]["median_ms"] / ev["inside_3"]["median_ms"], 4),
               "fill_z_over_inside_1": round(ev["fill_z"]["median_ms"] / ev["inside_1"]["median_ms"], 4),
               "fill_xyz_over_rows_xyz": round(ev["fill_xyz"]["median_ms"] / ev["rows_xyz"]["median_ms"], 3),
               "fill_z_over_rows_z": round(ev["fill_z"]["median_ms"] / ev["rows_z"]["median_ms"], 3),
               "margin_xyz_ms": round(spread("fill_xyz"), 5), "margin_z_ms": round(spread("fill_z"), 5),
               "stores_xyz_ms": round(ev["fill_xyz"]["median_ms"] - ev["rows_xyz"]["median_ms"], 5), "stores_z_ms": round(ev["fill_z"]["median_ms"] - ev["rows_z"]["median_ms"], 5),
               "faster_than_inside_3": bool(ev["fill_xyz"]["median_ms"] < ev["inside_3"]["median_ms"]),
               "explained_by_rows_xyz": bool(ev["fill_xyz"]["median_ms"] <= ev["rows_xyz"]["median_ms"] + spread("fill_xyz")),
               "explained_by_rows_z": bool(ev["fill_z"]["median_ms"] <= ev["rows_z"]["median_ms"] + spread("fill_z"))}
        result["scenes"][name]["lattices"][str(N)] = row
        print(json.dumps({name: {str(N): row}}), flush=True)
        for p in (d_rays, d_rec, d_in, d_ws, d_tot):
            mem.free(p)
    mem.free(d_tris)
    grid.free()

result["expectation_1_held"] = {s: {k: v["faster_than_inside_3"] for k, v in r["lattices"].items()} for s, r in result["scenes"].items()}
result["expectation_2_held"] = {s: {k: bool(v["explained_by_rows_xyz"] and v["explained_by_rows_z"]) for k, v in r["lattices"].items()} for s, r in result["scenes"].items()}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written to " + os.path.relpath(out_path, ROOT))
mem.close()
