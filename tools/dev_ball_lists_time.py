"""DEV TOOL: what ball lists cost (hagrid_ball_refs, hagrid_unique_lists, hagrid_compact_lists: hagrid_amd/csrc/ball_lists.hip) -- soup-1M and
the stadium mesh (0.95M triangles), default grid parameters, 2^20 queries uniform in the box enlarged by 10 % with r = 2 % of the diagonal: the case
tools/dev_nearest_k_time.py pages through with api.tris_within, and on the stadium mesh the case whose paging did not end within 60 s.

Per scene, in ONE process: the four launches of the protocol (count, fill, unique, compact) in their order, again and again after a warm-up, every launch
between its own pair of events on the context's stream and under its own time limit (a launch that does not come back within --limit seconds ends the process
with status 3: nothing else is started on the device); the scans are torch.cumsum outside the pairs.  Then api.ball_lists end to end on torch tensors (wall
clock around a synchronised call) and, in the same session, api.tris_within (untouched code; pages bounded by --max-pages, so on the mesh its lists are
prefixes and "complete" says so).  Recorded beside the times: references, triangles listed, the duplicate factor references / listed, the longest run of
references and the longest list, lists sorted in global memory, the scratch bytes (8 per reference).  If the references of all queries exceed --max-scratch-gb
the batch is halved until they fit, and "queries" says what was run.  Medians, nothing checked: no time was fixed in advance.

--ab LABEL: the A/B half instead -- what lost a kernel to the budget fold (hagrid_setup_traversal: wall clock around a synchronised call, image dropped in
between) and the two kernels whose header gained a neighbour (hagrid_closest_points, hagrid_nearest_tris at k = 8; 2^20 queries near the surface, r = inf),
alternating, medians; written to --out.  Run with HAGRID_AMD_LIB naming a build of the parent commit for the parent's half (it has no ball lists: nothing
else is touched).  --merge A1,B1,A2,B2 (this, parent, this, parent: the order they ran in) puts the four files into --out under "against_parent" with the
bar: each figure of this build (the mean of its two medians) within the mean of the parent's two medians plus the spread between them.

usage: python tools/dev_ball_lists_time.py [--queries 1048576] [--launches 7] [--warmup 1] [--limit 120] [--scenes soup,stadium] [--max-pages 64]
                                           [--max-scratch-gb 48] [--out profiles/ball_lists_time.json] [--ab LABEL] [--merge A1,B1,A2,B2]"""
import json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
nq = int(arg("--queries", str(1 << 20))); launches = int(arg("--launches", "7")); warmup = int(arg("--warmup", "1")); limit = float(arg("--limit", "120"))
scenes = arg("--scenes", "soup,stadium").split(","); max_pages = int(arg("--max-pages", "64")); max_scratch = float(arg("--max-scratch-gb", "48")) * (1 << 30)
out_path = arg("--out", os.path.join(ROOT, "profiles", "ball_lists_time.json"))
ab_label = arg("--ab", ""); merge = arg("--merge", "")


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


def write(result):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("written to " + os.path.relpath(out_path, ROOT))


if merge:
    files = merge.split(",")
    runs = [json.load(open(f)) for f in files]
    this, parent = [runs[0], runs[2]], [runs[1], runs[3]]
    rows = {}
    for name in this[0]["scenes"]:
        rows[name] = {}
        for fig in this[0]["scenes"][name]:
            p = [r["scenes"][name][fig]["median_ms"] for r in parent]; t = [r["scenes"][name][fig]["median_ms"] for r in this]
            bar = float(np.mean(p)) + abs(p[0] - p[1])
            rows[name][fig] = {"this_median_ms": t, "parent_median_ms": p, "bar_ms": round(bar, 5), "this_mean_ms": round(float(np.mean(t)), 5),
                               "within_bar": bool(np.mean(t) <= bar)}
    result = json.load(open(out_path)) if os.path.exists(out_path) else {"tool": "tools/dev_ball_lists_time.py"}
    result["against_parent"] = {"bar": "mean of this build's two medians <= mean of the parent's two medians + the spread between them", "order": "this, parent, this, parent",
                                "this_source_hash": this[0]["source_hash"], "parent_library": parent[0]["library"], "scenes": rows}
    write(result)
    sys.exit(0)


def make_scene(name):
    tris = scene.make_soup(1000000) if name == "soup" else scene.make_stadium()
    lo, hi = scene.tris_bbox(tris)
    return tris, lo, hi, scene.bbox_diagonal(lo, hi)


if ab_label and os.environ.get("HAGRID_AMD_LIB"):         # a build of the parent commit exports everything but the three entry points this tool is about
    from hagrid_amd import lib as _lib
    for symbol in ("hagrid_ball_refs", "hagrid_unique_lists", "hagrid_compact_lists"):
        _lib.SIGNATURES.pop(symbol, None)

mem = api.MemManager(keep=True)

if ab_label:
    result = {"tool": "tools/dev_ball_lists_time.py --ab", "label": ab_label, "library": os.path.relpath(os.environ["HAGRID_AMD_LIB"], ROOT) if os.environ.get("HAGRID_AMD_LIB") else "the tree's own", "source_hash": _build.source_hash(),
              "queries": nq, "launches": launches, "scenes": {}}
    for name in scenes:
        tris, lo, hi, diag = make_scene(name)
        d_tris = mem.upload(tris)
        grid = api.build_all(mem, d_tris, tris.shape[0])
        pts = np.empty((nq, 4), np.float32)
        pts[:, 0:3] = scene.make_points_near_surface(tris, lo, hi, nq, 101); pts[:, 3] = np.inf
        d_pts = mem.upload(pts); d_res = mem.alloc(32 * nq); d_ent = mem.alloc(8 * nq * 8)
        variants = [("closest_points", lambda: api.closest_points(grid, d_tris, d_pts, d_res, nq)),
                    ("nearest_tris_k8", lambda: api.nearest_tris(grid, d_tris, d_pts, nq, 8, entries=d_ent))]
        ms = {vn: [] for vn, _ in variants}
        ms["setup_traversal"] = []

        def setup():
            mem.set_option("traverse.image", 0); api.setup_traversal(grid)           # the image dropped
            mem.set_option("traverse.image", 2); mem.synchronize()
            t0 = time.perf_counter(); api.setup_traversal(grid); mem.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for it in range(warmup + launches):
            w = limited(setup, f"{name} setup_traversal")
            if it >= warmup:
                ms["setup_traversal"].append(w)
            for vn, fn in variants:
                t = limited(lambda: api.profile(fn, mem), f"{name} {vn}")
                if it >= warmup:
                    ms[vn].append(t)
        result["scenes"][name] = {vn: stats(v) for vn, v in ms.items()}
        result["scenes"][name]["setup_traversal"]["image_bytes"] = mem.image_bytes(grid)
        print(json.dumps({name: result["scenes"][name]}), flush=True)
        for p in (d_pts, d_res, d_ent, d_tris):
            mem.free(p)
        grid.free()
    write(result)
    mem.close()
    sys.exit(0)

import torch
mem.set_option("traverse.image", 0)
result = {"tool": "tools/dev_ball_lists_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "queries_asked": nq, "launches": launches, "warmup": warmup,
          "expectation": "stated before the first run: several times faster than api.tris_within on soup-1M; a run that finishes on the stadium mesh", "scenes": {}}
mem.use_stream(torch.cuda.current_stream().cuda_stream)
for name in scenes:
    tris, lo, hi, diag = make_scene(name)
    N = tris.shape[0]
    t_tris = torch.from_numpy(tris).cuda()
    d_tris = t_tris.data_ptr()
    grid = api.build_all(mem, d_tris, N)
    pts = np.empty((nq, 4), np.float32)
    pts[:, 0:3] = scene.make_points_uniform(lo, hi, nq, 102); pts[:, 3] = np.float32(0.02) * diag
    t_all = torch.from_numpy(pts).cuda()
    n = nq
    while True:                                     # the batch whose references fit the scratch bound
        t_pts = t_all[:n].contiguous()
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        limited(lambda: (api.ball_refs(grid, d_tris, t_pts.data_ptr(), n, counts=counts.data_ptr()), torch.cuda.synchronize()), f"{name} count (sizing)")
        refs = int(counts.sum(dtype=torch.int64).item())
        if refs * 8 <= max_scratch or n <= 1024:
            break
        n //= 2
    ro = torch.zeros(n + 1, dtype=torch.int64, device="cuda"); torch.cumsum(counts, 0, dtype=torch.int64, out=ro[1:])
    scratch = torch.empty((max(refs, 1), 2), dtype=torch.int32, device="cuda")
    m = torch.zeros(n, dtype=torch.int32, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    tot = {k: torch.zeros(6, dtype=torch.int64, device="cuda") for k in ("fill", "unique", "compact")}
    ms = {"count": [], "fill": [], "unique": [], "compact": []}
    out = None
    for it in range(warmup + launches):
        last = it == warmup + launches - 1
        t = [limited(lambda: api.profile(lambda: api.ball_refs(grid, d_tris, t_pts.data_ptr(), n, counts=counts.data_ptr()), mem), f"{name} count"),
             limited(lambda: api.profile(lambda: api.ball_refs(grid, d_tris, t_pts.data_ptr(), n, offsets=ro.data_ptr(), entries=scratch.data_ptr(), capacity=refs,
                                                               counters=tot["fill"].data_ptr() if last else 0), mem), f"{name} fill"),
             limited(lambda: api.profile(lambda: api.unique_lists(n, ro.data_ptr(), scratch.data_ptr(), refs, m.data_ptr(), counters=tot["unique"].data_ptr() if last else 0, mem=mem), mem),
                     f"{name} unique")]
        torch.cumsum(m, 0, dtype=torch.int64, out=off[1:])
        listed = int(off[-1].item())
        if out is None:
            out = torch.empty((max(listed, 1), 2), dtype=torch.int32, device="cuda")
        t.append(limited(lambda: api.profile(lambda: api.compact_lists(n, ro.data_ptr(), scratch.data_ptr(), refs, m.data_ptr(), off.data_ptr(), out.data_ptr(), listed,
                                                                      counters=tot["compact"].data_ptr() if last else 0, mem=mem), mem), f"{name} compact"))
        if it >= warmup:
            for k, v in zip(("count", "fill", "unique", "compact"), t):
                ms[k].append(v)
    row = {"triangles": int(N), "grid": grid.summary(), "queries": n, "radius_of_diagonal": 0.02, "stages": {k: stats(v) for k, v in ms.items()}}
    row["stages"]["sum_of_medians_ms"] = round(sum(row["stages"][k]["median_ms"] for k in ms), 5)
    f = tot["fill"].cpu().numpy(); u = tot["unique"].cpu().numpy()
    row.update({"references": refs, "listed": listed, "duplicate_factor": round(refs / max(listed, 1), 3), "scratch_bytes": 8 * refs, "output_bytes": 8 * listed,
                "longest_references": int(counts.max().item()), "longest_list": int(m.max().item()), "empty_lists": int((m == 0).sum().item()),
                "lists_sorted_in_global_memory": int(u[3]), "cells_per_query": round(f[1] / n, 2), "tris_per_query": round(f[2] / n, 2), "pruned_per_query": round(f[3] / n, 2)})
    del scratch, out
    walls = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        got = limited(lambda: api.ball_lists(grid, d_tris, t_pts), f"{name} ball_lists")
        torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
    row["ball_lists"] = {"wall_ms": [round(w, 3) for w in walls], "median_ms": round(float(np.median(walls)), 3), "listed": int(got["offsets"][-1].item()), "refs": got["refs"]}
    del got
    walls = []
    for _ in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        got = limited(lambda: api.tris_within(grid, d_tris, t_pts, k=8, max_pages=max_pages), f"{name} tris_within")
        torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
    row["tris_within_k8"] = {"wall_ms": [round(w, 3) for w in walls], "median_ms": round(float(np.median(walls)), 3), "listed": int(got["offsets"][-1].item()), "pages": got["pages"],
                             "complete": got["complete"], "max_pages": max_pages}
    row["ball_lists_over_tris_within"] = round(row["ball_lists"]["median_ms"] / row["tris_within_k8"]["median_ms"], 4)
    del got
    result["scenes"][name] = row
    print(json.dumps({name: row}), flush=True)
    grid.free()
    del t_pts, t_all, t_tris, counts, ro, m, off
    torch.cuda.empty_cache()
mem.use_stream(None)
if os.path.exists(out_path):                        # keep the A/B half a --merge left there
    old = json.load(open(out_path))
    if "against_parent" in old:
        result["against_parent"] = old["against_parent"]
write(result)
mem.close()
