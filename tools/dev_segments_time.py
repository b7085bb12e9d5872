"""DEV TOOL: what capsule queries cost (hagrid_segment_tris, segment_tris_kernel in hagrid_amd/csrc/capsule.hip) -- soup-1M and the
stadium mesh (0.95M triangles), default grid parameters, 2^20 segments of two kinds per scene:

  short    scene.make_segments_short: a near the surface, b = a + a Gaussian of 0.5 % of the box diagonal per axis, r = inf; k = 1 and k = 8
  long     scene.make_segments_diagonal: corner to corner, r = 2 % of the diagonal; k = 1

Beside each, what a caller had before the entry point existed: hagrid_nearest_tris at the segments' MIDPOINTS with r + length / 2 (for r = inf: inf).  Its
lists are not the answer (point distances, a ball that holds the capsule); it is there as a cost comparison only.  In ONE process and alternating after a
warm-up, every launch between its own pair of events on the context's stream and under its own time limit (a launch that does not come back within
--limit seconds ends the process with status 3: nothing else is started on the device).  Per launch kind one more launch with counters: cells visited,
triangles tested, sub-blocks pruned and full lists per query.  Nothing is checked: no time was fixed in advance.  Written to --out (default
profiles/segments_time.json) with build.source_hash().

usage: python tools/dev_segments_time.py [--queries 1048576] [--launches 9] [--warmup 1] [--limit 120] [--scenes soup,stadium] [--out profiles/segments_time.json]"""
import json, os, sys, threading
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
nq = int(arg("--queries", str(1 << 20))); launches = int(arg("--launches", "9")); warmup = int(arg("--warmup", "1")); limit = float(arg("--limit", "120"))
scenes = arg("--scenes", "soup,stadium").split(",")
out_path = arg("--out", os.path.join(ROOT, "profiles", "segments_time.json"))


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


def midpoints(s):
    """the workaround's queries: the midpoint with r + length / 2"""
    d = s[:, 4:7] - s[:, 0:3]
    p = np.empty((s.shape[0], 4), np.float32)
    p[:, 0:3] = s[:, 0:3] + d * np.float32(0.5)
    p[:, 3] = s[:, 3] + np.sqrt((d * d).sum(axis=1, dtype=np.float32)) * np.float32(0.5)
    return p


mem = api.MemManager(keep=True)
mem.set_option("traverse.image", 0)
result = {"tool": "tools/dev_segments_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "queries": nq, "launches": launches, "warmup": warmup,
          "scenes": {}}
for name in scenes:
    tris = scene.make_soup(1000000) if name == "soup" else scene.make_stadium()
    N = tris.shape[0]
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, N)
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    segs = {"short": scene.make_segments_short(tris, lo, hi, nq, 201), "long": scene.make_segments_diagonal(lo, hi, nq, 202, r=np.float32(0.02) * diag)}
    d_ent = mem.alloc(8 * nq * 8); d_cnt = mem.alloc(40)
    row = {"triangles": int(N), "grid": grid.summary(), "kinds": {}}
    for kind, ks in (("short", (1, 8)), ("long", (1,))):
        d_seg = mem.upload(segs[kind]); d_mid = mem.upload(midpoints(segs[kind]))
        variants = []
        for k in ks:
            variants.append((f"segment_k{k}", lambda c=0, k=k: api.segment_tris(grid, d_tris, d_seg, nq, k, entries=d_ent, counters=c)))
            variants.append((f"midpoint_k{k}", lambda c=0, k=k: api.nearest_tris(grid, d_tris, d_mid, nq, k, entries=d_ent, counters=c)))
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
            out[vn] = dict(stats(ms[vn]), cells_per_query=round(c[1] / nq, 2), tris_per_query=round(c[2] / nq, 2), pruned_per_query=round(c[3] / nq, 2), full_lists=int(c[4]))
        row["kinds"][kind] = out
        mem.free(d_seg); mem.free(d_mid)
    result["scenes"][name] = row
    print(json.dumps({name: row}), flush=True)
    for p in (d_ent, d_cnt, d_tris):
        mem.free(p)
    grid.free()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written to " + os.path.relpath(out_path, ROOT))
mem.close()
