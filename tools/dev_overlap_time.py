"""DEV TOOL: what box-overlap queries cost (hagrid_overlap_boxes, hagrid_overlap_lattice, hagrid_amd/csrc/overlap.hip) -- soup-1M and the stadium mesh
(0.95M triangles), default grid parameters.  Per scene:

  boxes    2^20 boxes with an edge of 1 % of the box diagonal, centred on near-surface points (surface samples moved by a Gaussian of 1 % of the diagonal):
           k = 1, k = 8 and ANY
  lattice  a 256^3 lattice over the scene box: k = 1 and ANY
  sphere   what a caller has to use without the box query: hagrid_closest_points on the box centres with r = half the box's own diagonal
  nearest  the control of tools/dev_closest_time.py: the nearest-hit launch over the same construction format on 1024 x 1024 primary rays
  contact  hagrid_overlap_tris (the contact mode of the same kernel), k = 8 and ANY, over two batches of min(triangles, boxes) query triangles: `own`, the
           scene's own array with its labels (the mesh's index triples; the soup's triangles carry their own number), and `moved`, a copy of those triangles
           moved by 1 % of the diagonal, without labels -- each alternating in the same run with hagrid_overlap_boxes over the same triangles' grown
           bounding boxes (scene.query_boxes) at the same k: the ratio contact / boxes and the totals per query

ONE process, the launches alternating after a warm-up, every launch between its own pair of events on the context's stream and under its own time limit (a
launch that does not come back within --limit seconds ends the process with status 3: nothing else is started on the device).  Per box launch one more with
the batch totals: cells visited, triangle / box tests and sub-blocks pruned per box.  The expectation stated beforehand: boxes k = 1 is no slower than
sphere, the margin being the spread of sphere in this run (p90 - median); the outcome is recorded, nothing is asserted.  Written to --out (default
profiles/overlap_time.json) with build.source_hash().  --parent FILE: the file the same tool wrote when run on the parent commit; the box launches of this
run are set against it under the expectation stated beforehand -- no slower than the parent's, the margin being the parent run's own spread (p90 - median) --
and the outcome is recorded.

usage: python tools/dev_overlap_time.py [--boxes 1048576] [--lattice 256] [--launches 20] [--warmup 3] [--limit 60] [--scenes soup,stadium] [--out profiles/overlap_time.json] [--parent FILE]"""
import json, os, sys, threading
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
nb = int(arg("--boxes", str(1 << 20))); lat = int(arg("--lattice", "256")); launches = int(arg("--launches", "20")); warmup = int(arg("--warmup", "3"))
limit = float(arg("--limit", "60"))
scenes = arg("--scenes", "soup,stadium").split(",")
out_path = arg("--out", os.path.join(ROOT, "profiles", "overlap_time.json"))
parent_path = arg("--parent", "")


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
result = {"tool": "tools/dev_overlap_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "boxes": nb, "lattice": lat, "launches": launches,
          "warmup": warmup, "scenes": {}}
nv = lat ** 3
W = 1024
for name in scenes:
    if name == "soup":
        tris = scene.make_soup(1000000)
        labels = np.full((tris.shape[0], 3), -1, np.int32); labels[:, 0] = np.arange(tris.shape[0])
    else:
        verts, faces = scene.make_stadium_mesh()
        tris = scene.tris_from_mesh(verts, faces); labels = np.ascontiguousarray(faces, np.int32)
    N = tris.shape[0]
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, N); api.setup_traversal(grid)
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    edge = np.float32(0.01) * diag
    centres = scene.make_points_near_surface(tris, lo, hi, nb, 101)
    boxes = np.zeros((nb, 8), np.float32)
    boxes[:, 0:3] = centres - np.float32(0.5) * edge; boxes[:, 4:7] = centres + np.float32(0.5) * edge
    pts = np.empty((nb, 4), np.float32)
    pts[:, 0:3] = centres; pts[:, 3] = np.float32(0.5) * np.float32(np.sqrt(np.float32(3.0))) * edge
    d_boxes = mem.upload(boxes); d_pts = mem.upload(pts)
    most = max(8 * nb, nv)
    d_ids = mem.alloc(4 * most); d_counts = mem.alloc(4 * max(nb, nv)); d_res = mem.alloc(32 * nb); d_tot = mem.alloc(32)
    origin = lo; size = ((hi - lo) / np.float32(lat)).astype(np.float32); n3 = (lat, lat, lat)
    ANY = api.OVERLAP_ANY
    cam = scene.camera(grid.bbox_min, grid.bbox_max)
    d_rays = mem.alloc(32 * W * W); d_hits = mem.alloc(16 * W * W)
    api.gen_primary_rays(mem, cam, float(cam[4]), W, W, d_rays)
    variants = [("nearest", lambda: api.traverse_grid(grid, d_tris, d_rays, d_hits, W * W)),
                ("sphere", lambda: api.closest_points(grid, d_tris, d_pts, d_res, nb)),
                ("boxes_k1", lambda: api.overlap_boxes(grid, d_tris, d_boxes, nb, 1, d_ids, d_counts)),
                ("boxes_k8", lambda: api.overlap_boxes(grid, d_tris, d_boxes, nb, 8, d_ids, d_counts)),
                ("boxes_any", lambda: api.overlap_boxes(grid, d_tris, d_boxes, nb, 1, d_ids, d_counts, 0, ANY)),
                ("lattice_k1", lambda: api.voxelize(grid, d_tris, origin, size, n3, 1, d_ids, d_counts)),
                ("lattice_any", lambda: api.voxelize(grid, d_tris, origin, size, n3, 1, d_ids, d_counts, 0, ANY))]
    # contact queries: the scene's own triangles with labels, and a moved copy; beside each the box query over the same triangles' grown bounding boxes
    nq = min(N, nb)
    moved = tris[:nq].copy()
    moved[:, 0:3] = (moved[:, 0:3] + np.float32(0.01) * diag * np.float32(0.57735026)).astype(np.float32)
    d_labels = mem.upload(labels); d_moved = mem.upload(moved)
    d_box_own = mem.upload(scene.query_boxes(tris[:nq], grid.bbox_min, grid.bbox_max)); d_box_moved = mem.upload(scene.query_boxes(moved, grid.bbox_min, grid.bbox_max))
    contact = {}
    for qn, d_q, d_b, lab in (("own", d_tris, d_box_own, d_labels), ("moved", d_moved, d_box_moved, 0)):
        for kn, k, fl in (("k8", 8, 0), ("any", 1, ANY)):
            contact[f"tris_{qn}_{kn}"] = (lambda t=0, d_q=d_q, lab=lab, k=k, fl=fl: api.overlap_tris(grid, d_tris, d_q, nq, k, d_ids, d_counts, t, fl, query_labels=lab, tri_labels=lab))
            contact[f"qboxes_{qn}_{kn}"] = (lambda t=0, d_b=d_b, k=k, fl=fl: api.overlap_boxes(grid, d_tris, d_b, nq, k, d_ids, d_counts, t, fl))
    variants += list(contact.items())
    for _ in range(warmup):
        for vn, fn in variants:
            limited(lambda: (fn(), mem.synchronize()), f"{name} {vn} (warm-up)")
    ms = {vn: [] for vn, _ in variants}
    for _ in range(launches):
        for vn, fn in variants:                                   # alternating: one launch of each, in turn
            ms[vn].append(limited(lambda: api.profile(fn, mem), f"{name} {vn}"))
    ev = {k: stats(v) for k, v in ms.items()}
    spread = ev["sphere"]["p90_ms"] - ev["sphere"]["median_ms"]
    row = {"triangles": int(N), "grid": grid.summary(), "box_edge": float(edge), "sphere_radius": float(pts[0, 3]), "events": ev,
           "expectation": {"boxes_k1_median_ms": ev["boxes_k1"]["median_ms"], "sphere_median_ms": ev["sphere"]["median_ms"], "margin_ms": round(spread, 5),
                           "holds": bool(ev["boxes_k1"]["median_ms"] <= ev["sphere"]["median_ms"] + spread)}, "kinds": {}}
    totals = [("boxes_k1", nb, lambda t: api.overlap_boxes(grid, d_tris, d_boxes, nb, 1, d_ids, d_counts, t)),
              ("boxes_k8", nb, lambda t: api.overlap_boxes(grid, d_tris, d_boxes, nb, 8, d_ids, d_counts, t)),
              ("boxes_any", nb, lambda t: api.overlap_boxes(grid, d_tris, d_boxes, nb, 1, d_ids, d_counts, t, ANY)),
              ("lattice_k1", nv, lambda t: api.voxelize(grid, d_tris, origin, size, n3, 1, d_ids, d_counts, t)),
              ("lattice_any", nv, lambda t: api.voxelize(grid, d_tris, origin, size, n3, 1, d_ids, d_counts, t, ANY))]
    totals += [(vn, nq, fn) for vn, fn in contact.items()]
    for vn, n, fn in totals:
        mem.zero(d_tot, 32)
        limited(lambda: (fn(d_tot), mem.synchronize()), f"{name} {vn} (totals)")
        c = mem.download(d_tot, np.int64, 4)
        cnt = mem.download(d_counts, np.int32, n)
        t = ev[vn]["median_ms"]
        row["kinds"][vn] = {"median_ms": t, "Mboxes_per_s": round(n / t / 1e3, 1), "non_empty": int((cnt > 0).sum()), "more_than_k": int((cnt > (8 if vn.endswith("k8") else 1)).sum()),
                            "cells_per_box": round(c[1] / n, 3), "tests_per_box": round(c[2] / n, 3), "pruned_per_box": round(c[3] / n, 3),
                            "ns_per_test": round(t * 1e6 / max(int(c[2]), 1), 4), "ns_per_cell": round(t * 1e6 / max(int(c[1]), 1), 4)}
    mem.zero(d_tot, 32)
    limited(lambda: (api.closest_points(grid, d_tris, d_pts, d_res, nb, d_tot), mem.synchronize()), f"{name} sphere (totals)")
    c = mem.download(d_tot, np.int64, 4)
    t = ev["sphere"]["median_ms"]
    row["kinds"]["sphere"] = {"median_ms": t, "Mqueries_per_s": round(nb / t / 1e3, 1), "found": int((mem.download(d_res, api.CLOSEST_DTYPE, nb)["id"] >= 0).sum()),
                              "cells_per_query": round(c[1] / nb, 3), "tris_per_query": round(c[2] / nb, 3), "pruned_per_query": round(c[3] / nb, 3)}
    row["contact"] = {"queries": int(nq), "moved_by": float(np.float32(0.01) * diag)}
    for qn in ("own", "moved"):
        for kn in ("k8", "any"):
            t, b = row["kinds"][f"tris_{qn}_{kn}"], row["kinds"][f"qboxes_{qn}_{kn}"]
            row["contact"][f"{qn}_{kn}"] = {"tris_median_ms": t["median_ms"], "boxes_median_ms": b["median_ms"], "ratio_tris_to_boxes": round(t["median_ms"] / b["median_ms"], 4),
                                            "contacts_non_empty": t["non_empty"], "boxes_non_empty": b["non_empty"], "pairs_offered_per_query": t["tests_per_box"],
                                            "box_tests_per_query": b["tests_per_box"], "cells_per_query": t["cells_per_box"]}
    if parent_path:
        pr = json.load(open(parent_path))["scenes"].get(name)
        if pr:
            row["against_parent"] = {"parent_source_hash": json.load(open(parent_path)).get("source_hash"), "expectation": "the box launches are no slower than the parent's; margin: the parent run's p90 - median"}
            for vn in ("boxes_k1", "boxes_k8", "boxes_any", "lattice_k1", "lattice_any"):
                pe = pr["events"][vn]; margin = pe["p90_ms"] - pe["median_ms"]
                row["against_parent"][vn] = {"median_ms": ev[vn]["median_ms"], "parent_median_ms": pe["median_ms"], "margin_ms": round(margin, 5),
                                             "ratio": round(ev[vn]["median_ms"] / pe["median_ms"], 4), "holds": bool(ev[vn]["median_ms"] <= pe["median_ms"] + margin)}
    result["scenes"][name] = row
    print(json.dumps({name: row}), flush=True)
    for p in (d_boxes, d_pts, d_ids, d_counts, d_res, d_tot, d_rays, d_hits, d_tris, d_labels, d_moved, d_box_own, d_box_moved):
        mem.free(p)
    grid.free()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("written to " + os.path.relpath(out_path, ROOT))
mem.close()
