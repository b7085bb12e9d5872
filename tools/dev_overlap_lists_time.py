"""DEV TOOL: what overlap lists cost (hagrid_box_refs, hagrid_tri_refs, hagrid_obb_refs, then hagrid_unique_lists and hagrid_compact_lists:
hagrid_amd/csrc/overlap_lists.hip) against paging the k-list queries -- soup-1M and the stadium mesh (0.95M triangles), default grid parameters.

Per scene, in ONE process, three cases:
  planks    the --planks (default 1024; 0: leave the case out) thin diagonal planks of tools/dev_obb_time.py: api.obb_lists against api.tris_in_obbs
            (untouched code); the case runs last: on soup-1M one walk of it takes 24 s and paging it does not end within 200 s
  small     --queries (default 2^20) rotated boxes with half extents of 0.5 % of the diagonal near the surface (tools/dev_obb_time.py's): the same pair
  contacts  --queries labelled contact queries (the scene's own triangles in a shuffled order, their own labels): api.contact_lists against overlap_tris at
            k = 8 paged to the end (first = last id + 1 for the lists that came back full)
For each case the four launches of the protocol (count, fill, unique, compact) in their order, again and again after a warm-up, every launch between its own
pair of events on the context's stream and under its own time limit (a launch that does not come back within --limit seconds ends the process with status 3:
nothing else is started on the device); the scans are torch.cumsum outside the pairs.  Then the api function end to end on torch tensors (wall clock around a
synchronised call) and, in the same session, the paged form (pages bounded by --max-pages; "complete" says whether that sufficed).  Recorded beside the
times: references, triangles listed, the duplicate factor references / listed, the longest run of references and the longest list, lists sorted in global
memory, the scratch bytes (8 per reference).  Medians, nothing checked: the expectation is written down in DESIGN.md 4.18.

--ab LABEL: the A/B half instead -- what lost two kernels to the budget fold (expand_select of expand.hip: one kernel with the axis as an argument): for
soup-1M and soup-8M (compressed) the expansion alone (hagrid_expand_grid between events on a freshly built, merged and flattened grid) and the whole
construction (wall clock around a synchronised build_all), medians; written to --out.  Run with HAGRID_AMD_LIB naming a build of the parent commit for the
parent's half.  --merge A1,B1,A2,B2 (this, parent, this, parent: the order they ran in) puts the four files into --out under "against_parent" with the bar:
each figure of this build (the mean of its two medians) within the mean of the parent's two medians plus the spread between them.

usage: python tools/dev_overlap_lists_time.py [--queries 1048576] [--planks 1024] [--launches 7] [--warmup 1] [--limit 120] [--scenes soup,stadium]
                                              [--max-pages 4096] [--out profiles/overlap_lists_time.json] [--ab LABEL] [--merge A1,B1,A2,B2]"""
import json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
nq = int(arg("--queries", str(1 << 20))); npl = int(arg("--planks", "1024")); launches = int(arg("--launches", "7")); warmup = int(arg("--warmup", "1"))
limit = float(arg("--limit", "120")); scenes = arg("--scenes", "soup,stadium").split(","); max_pages = int(arg("--max-pages", "4096"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "overlap_lists_time.json"))
ab_label = arg("--ab", ""); merge = arg("--merge", "")


def limited(fn, what):
    """fn() under its own time limit"""
    def expired():
        print(f"TIME LIMIT: {what} did not finish within {limit} s", flush=True)
        os._exit(3)
    t = threading.Timer(limit, expired); t.daemon = True; t.start()
    t0 = time.perf_counter()
    try:
        return fn()
    finally:
        t.cancel()
        print(f"  {what}: {(time.perf_counter() - t0) * 1e3:.1f} ms of wall clock", flush=True)      # (a long run stays visibly alive)


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
    runs = [json.load(open(f)) for f in merge.split(",")]
    this, parent = [runs[0], runs[2]], [runs[1], runs[3]]
    for r in this + parent:                             # an A/B merged in the wrong order would compare a build with itself
        own = r["library"] == "the tree's own"
        assert own == (r in this), f"--merge takes this, parent, this, parent: {r['label']} ran with {r['library']}"
    rows = {}
    for name in this[0]["scenes"]:
        rows[name] = {}
        for fig in this[0]["scenes"][name]:
            p = [r["scenes"][name][fig]["median_ms"] for r in parent]; t = [r["scenes"][name][fig]["median_ms"] for r in this]
            bar = float(np.mean(p)) + abs(p[0] - p[1])
            rows[name][fig] = {"this_median_ms": t, "parent_median_ms": p, "bar_ms": round(bar, 5), "this_mean_ms": round(float(np.mean(t)), 5),
                               "within_bar": bool(np.mean(t) <= bar)}
    result = json.load(open(out_path)) if os.path.exists(out_path) else {"tool": "tools/dev_overlap_lists_time.py"}
    result["against_parent"] = {"bar": "mean of this build's two medians <= mean of the parent's two medians + the spread between them", "order": "this, parent, this, parent",
                                "this_source_hash": this[0]["source_hash"], "parent_library": parent[0]["library"], "scenes": rows}
    write(result)
    sys.exit(0)

if ab_label and os.environ.get("HAGRID_AMD_LIB"):         # a build of the parent commit exports everything but the three entry points this tool is about
    from hagrid_amd import lib as _lib
    for symbol in ("hagrid_box_refs", "hagrid_tri_refs", "hagrid_obb_refs"):
        _lib.SIGNATURES.pop(symbol, None)

mem = api.MemManager(keep=True)

if ab_label:
    result = {"tool": "tools/dev_overlap_lists_time.py --ab", "label": ab_label, "library": os.path.relpath(os.environ["HAGRID_AMD_LIB"], ROOT) if os.environ.get("HAGRID_AMD_LIB") else "the tree's own",
              "source_hash": _build.source_hash(), "launches": launches, "scenes": {}}
    for name, count, compress in (("soup-1M", 1000000, False), ("soup-8M", 8000000, True)):
        tris = scene.make_soup(count)
        d_tris = mem.upload(tris)
        ms = {"expand_grid": [], "build_all_wall": []}
        for it in range(warmup + launches):
            grid = api.Grid()
            api.build_grid(mem, d_tris, count, grid, 0.12, 2.4); api.merge_grid(mem, grid, 0.995); api.flatten_grid(mem, grid)
            mem.synchronize()
            t = limited(lambda: api.profile(lambda: api.expand_grid(mem, grid, d_tris, 3), mem), f"{name} expand_grid")
            grid.free()
            mem.synchronize(); t0 = time.perf_counter()
            grid = limited(lambda: api.build_all(mem, d_tris, count, compress=compress), f"{name} build_all"); mem.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            cells = grid.num_cells
            grid.free()
            if it >= warmup:
                ms["expand_grid"].append(t); ms["build_all_wall"].append(w)
        result["scenes"][name] = {k: stats(v) for k, v in ms.items()}
        result["scenes"][name]["expand_grid"]["cells"] = int(cells)
        print(json.dumps({name: result["scenes"][name]}), flush=True)
        mem.free(d_tris)
    write(result)
    mem.close()
    sys.exit(0)

import torch
mem.set_option("traverse.image", 0)
result = {"tool": "tools/dev_overlap_lists_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "queries_asked": nq, "planks": npl, "launches": launches,
          "warmup": warmup, "expectation": "stated before the first run: faster than paging wherever lists exceed one page (8 ids)", "scenes": {}}
mem.use_stream(torch.cuda.current_stream().cuda_stream)


def page_contacts(grid, d_tris, t_q, t_lab, t_tl):
    """overlap_tris at k = 8 paged to the end: (triangles listed, pages, complete)"""
    n = int(t_q.shape[0]); k = 8
    q, lab = t_q, t_lab
    first = torch.zeros(n, dtype=torch.int32, device="cuda")
    listed, pages = 0, 0
    while q.shape[0]:
        if pages >= max_pages:
            return listed, pages, False
        pages += 1
        m = int(q.shape[0])
        ids = torch.empty((m, k), dtype=torch.int32, device="cuda"); counts = torch.empty(m, dtype=torch.int32, device="cuda")
        api.overlap_tris(grid, d_tris, q.data_ptr(), m, k, ids.data_ptr(), counts.data_ptr(), first=first.data_ptr(), query_labels=lab.data_ptr(), tri_labels=t_tl.data_ptr())
        more = counts > k
        listed += int((ids >= 0).sum().item())
        if int(more.sum().item()) == 0:
            break
        q, lab, first = q[more].contiguous(), lab[more].contiguous(), (ids[more][:, k - 1] + 1).contiguous()
    return listed, pages, True


for name in scenes:
    print("scene " + name, flush=True)
    tris = scene.make_soup(1000000) if name == "soup" else scene.make_stadium()
    lo, hi = scene.tris_bbox(tris); diag = scene.bbox_diagonal(lo, hi)
    N = tris.shape[0]
    t_tris = torch.from_numpy(tris).cuda()
    d_tris = t_tris.data_ptr()
    grid = api.build_all(mem, d_tris, N)
    h = np.float32(0.005) * diag
    R = scene.make_rotations(201, nq)
    small = scene.make_obbs(scene.make_points_near_surface(tris, lo, hi, nq, 101), R[:, :, 0] * h, R[:, :, 1] * h, R[:, :, 2] * h)
    planks = scene.make_obb_planks(lo, hi, max(npl, 1), 202)
    labels = np.full((N, 3), -1, np.int32); labels[:, 0] = np.arange(N)
    if name != "soup":
        labels = np.ascontiguousarray(scene.make_stadium_mesh()[1], np.int32)
    pick = np.random.default_rng(7).permutation(N)[:min(nq, N)] if nq < N else np.random.default_rng(7).integers(0, N, nq)
    t_tl = torch.from_numpy(labels).cuda()
    t_cq = t_tris[torch.from_numpy(pick).cuda()].contiguous(); t_cl = t_tl[torch.from_numpy(pick).cuda()].contiguous()
    rows = {"triangles": int(N), "grid": grid.summary(), "cases": {}}
    cases = (("small", torch.from_numpy(np.ascontiguousarray(small).view(np.float32).reshape(-1, 16)).cuda()),
             ("contacts", t_cq),
             ("planks", torch.from_numpy(np.ascontiguousarray(planks).view(np.float32).reshape(-1, 16)).cuda()))[:3 if npl else 2]       # --planks 0: without them
    for case, t_rec in cases:
        n = int(t_rec.shape[0])
        if case == "contacts":
            stage1 = lambda **kw: api.tri_refs(grid, d_tris, t_rec.data_ptr(), n, query_labels=t_cl.data_ptr(), tri_labels=t_tl.data_ptr(), **kw)
            whole = lambda: api.contact_lists(grid, d_tris, t_rec, query_labels=t_cl, tri_labels=t_tl)
        else:
            stage1 = lambda **kw: api.obb_refs(grid, d_tris, t_rec.data_ptr(), n, **kw)
            whole = lambda: api.obb_lists(grid, d_tris, t_rec)
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        limited(lambda: (stage1(counts=counts.data_ptr()), torch.cuda.synchronize()), f"{name} {case} count (sizing)")
        refs = int(counts.sum(dtype=torch.int64).item())
        ro = torch.zeros(n + 1, dtype=torch.int64, device="cuda"); torch.cumsum(counts, 0, dtype=torch.int64, out=ro[1:])
        longest_refs = int(counts.max().item())
        scratch = torch.empty((max(refs, 1), 2), dtype=torch.int32, device="cuda")
        m = torch.zeros(n, dtype=torch.int32, device="cuda"); off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        tot = {k: torch.zeros(6, dtype=torch.int64, device="cuda") for k in ("fill", "unique")}
        ms = {"count": [], "fill": [], "unique": [], "compact": []}
        out = None
        for it in range(warmup + launches):
            last = it == warmup + launches - 1
            t = [limited(lambda: api.profile(lambda: stage1(counts=counts.data_ptr()), mem), f"{name} {case} count"),
                 limited(lambda: api.profile(lambda: stage1(offsets=ro.data_ptr(), entries=scratch.data_ptr(), capacity=refs, counters=tot["fill"].data_ptr() if last else 0), mem),
                         f"{name} {case} fill"),
                 limited(lambda: api.profile(lambda: api.unique_lists(n, ro.data_ptr(), scratch.data_ptr(), refs, m.data_ptr(), counters=tot["unique"].data_ptr() if last else 0, mem=mem), mem),
                         f"{name} {case} unique")]
            torch.cumsum(m, 0, dtype=torch.int64, out=off[1:])
            listed = int(off[-1].item())
            if out is None:
                out = torch.empty((max(listed, 1), 2), dtype=torch.int32, device="cuda")
            t.append(limited(lambda: api.profile(lambda: api.compact_lists(n, ro.data_ptr(), scratch.data_ptr(), refs, m.data_ptr(), off.data_ptr(), out.data_ptr(), listed, mem=mem), mem),
                             f"{name} {case} compact"))
            if it >= warmup:
                for k, v in zip(("count", "fill", "unique", "compact"), t):
                    ms[k].append(v)
        row = {"queries": n, "stages": {k: stats(v) for k, v in ms.items()}}
        row["stages"]["sum_of_medians_ms"] = round(sum(row["stages"][k]["median_ms"] for k in ms), 5)
        f = tot["fill"].cpu().numpy(); u = tot["unique"].cpu().numpy()
        row.update({"references": refs, "listed": listed, "duplicate_factor": round(refs / max(listed, 1), 3), "scratch_bytes": 8 * refs, "output_bytes": 8 * listed,
                    "longest_references": longest_refs, "longest_list": int(m.max().item()), "empty_lists": int((m == 0).sum().item()),
                    "lists_longer_than_one_page": int((m > 8).sum().item()), "lists_sorted_in_global_memory": int(u[3]),
                    "cells_per_query": round(f[1] / n, 2), "tests_per_query": round(f[2] / n, 2), "pruned_per_query": round(f[3] / n, 2)})
        del scratch, out
        walls = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            got = limited(whole, f"{name} {case} lists")
            torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
        row["lists"] = {"wall_ms": [round(w, 3) for w in walls], "median_ms": round(float(np.median(walls)), 3), "listed": int(got["offsets"][-1].item()), "refs": got["refs"]}
        del got
        walls = []
        for _ in range(2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            if case == "contacts":
                p_listed, pages, complete = limited(lambda: page_contacts(grid, d_tris, t_rec, t_cl, t_tl), f"{name} {case} paging")
            else:
                got = limited(lambda: api.tris_in_obbs(grid, d_tris, t_rec, k=8, max_pages=max_pages), f"{name} {case} tris_in_obbs")
                p_listed, pages, complete = int(got["offsets"][-1].item()), got["pages"], got["complete"]
                del got
            torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
        row["paged_k8"] = {"wall_ms": [round(w, 3) for w in walls], "median_ms": round(float(np.median(walls)), 3), "listed": p_listed, "pages": pages, "complete": complete,
                           "max_pages": max_pages}
        row["lists_over_paged"] = round(row["lists"]["median_ms"] / row["paged_k8"]["median_ms"], 4)
        rows["cases"][case] = row
        print(json.dumps({name: {case: row}}), flush=True)
        del counts, ro, m, off
        torch.cuda.empty_cache()
    result["scenes"][name] = rows
    grid.free()
    del t_tris, t_tl, t_cq, t_cl, cases
    torch.cuda.empty_cache()
mem.use_stream(None)
if os.path.exists(out_path):                        # keep the A/B half a --merge left there
    old = json.load(open(out_path))
    if "against_parent" in old:
        result["against_parent"] = old["against_parent"]
write(result)
mem.close()
