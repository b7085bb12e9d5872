"""DEV TOOL: what it costs to make build_grid's input on the device (hagrid_scene_assemble, hagrid_amd/csrc/assemble.hip) instead of uploading it --
four scenes, in ONE process, warm, the variants alternating launch by launch:

  stadium_one       scene.make_stadium_mesh (0.95M triangles, shared vertices) as one instance without a transform
  stadium_objects   the same mesh split into its objects (connected index ranges), one instance and one matrix each
  soup_1M           soup-1M as vertices without indices (triangle p = vertices 3p, 3p+1, 3p+2)
  dust              10^5 instances of 2 .. 20 triangles each, a matrix each: nearly every wavefront straddles instances (the per-lane search)

Per scene, medians:
  assemble_ms       the assemble launch between its own pair of events on the context's stream
  upload_ms         what it replaces: MemManager.upload of the host-made Tri array of the same scene (the only route before), a host clock around
                    the synchronous copy (pool allocation included, the buffer returned to the pool afterwards)
  bytes             the launch's compulsory bytes: 12 per index triple, the vertex bytes once, 48 per triangle out, 48 per instance of matrix;
                    over assemble_ms as a share of the copy rate hagrid_bandwidth_probe measures in the same run
  assemble_build_grid_ms   assemble + hagrid_build_grid (which reads the records next), host clock: the figure to compare store variants on
  new_vertices_to_first_ray_ms   (stadium_objects) assemble + build_all + setup_traversal, host clock

One condition is checked: on the three scenes of 10^6 triangles of a user's kind (all but dust) the assemble launch takes less time than the upload
(the exit status says so).  Written to --out (default profiles/assemble_time.json) with build.source_hash().

usage: python tools/dev_assemble_time.py [--frames 60] [--warmup 5] [--out profiles/assemble_time.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build, lib as _lib

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
frames = int(arg("--frames", "60")); warmup = int(arg("--warmup", "5"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "assemble_time.json"))


def split_objects(V, F):
    """the connected index ranges of a mesh whose objects were appended one after the other: [(vertices, faces)]"""
    top = np.maximum.accumulate(F.max(axis=1))
    starts = np.concatenate([[0], 1 + np.flatnonzero(F.min(axis=1)[1:] > top[:-1]), [F.shape[0]]])
    out = []
    for a, b in zip(starts[:-1], starts[1:]):
        lo, hi = int(F[a:b].min()), int(F[a:b].max()) + 1
        out.append((np.ascontiguousarray(V[lo:hi]), np.ascontiguousarray(F[a:b] - lo)))
    return out


def small_turns(n, seed):
    """n matrices close to the identity: a turn of up to 0.02 rad about y, a scale within 1 %, a shift of up to 0.002"""
    u = scene.uniform01(seed, np.arange(3 * n, dtype=np.uint64)).reshape(n, 3).astype(np.float64)
    a = 0.02 * (u[:, 0] - 0.5); s = 1.0 + 0.01 * (u[:, 1] - 0.5); t = 0.002 * (u[:, 2] - 0.5)
    M = np.zeros((n, 3, 4))
    M[:, 0, 0] = s * np.cos(a); M[:, 0, 2] = s * np.sin(a); M[:, 1, 1] = s; M[:, 2, 0] = -s * np.sin(a); M[:, 2, 2] = s * np.cos(a); M[:, :, 3] = t[:, None]
    return M.reshape(n, 12).astype(np.float32)


def scenes():
    V, F = scene.make_stadium_mesh()
    yield "stadium_one", [(V, F)], None, None
    objs = split_objects(V, F)
    yield "stadium_objects", objs, None, small_turns(len(objs), 5)
    soup = scene.make_soup(1_000_000)
    sv = np.ascontiguousarray(np.stack([soup[:, 0:3], soup[:, 0:3] - soup[:, 4:7], soup[:, 0:3] + soup[:, 8:11]], axis=1).reshape(-1, 3), np.float32)
    yield "soup_1M", [(sv, None, soup.shape[0])], None, None
    n_inst = 100_000
    small = []
    for k in range(2, 21):
        u = scene.uniform01(100 + k, np.arange(9 * k, dtype=np.uint64)).reshape(3 * k, 3)
        small.append((np.ascontiguousarray(u, np.float32), None, k))
    u = scene.uniform01(7, np.arange(3 * n_inst, dtype=np.uint64)).reshape(n_inst, 3)
    M = np.zeros((n_inst, 3, 4), np.float32)
    M[:, 0, 0] = M[:, 1, 1] = M[:, 2, 2] = np.float32(0.004); M[:, :, 3] = u
    yield "dust", small, (np.arange(n_inst) * 7 % 19).tolist(), M.reshape(n_inst, 12)


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 5), "min_ms": round(float(a[0]), 5), "p90_ms": round(float(a[int(0.9 * (a.size - 1))]), 5)}


mem = api.MemManager(keep=True)
probe = mem.bandwidth_probe(1 << 30, 5)
result = {"tool": "tools/dev_assemble_time.py", "source_hash": _build.source_hash(), "library": os.path.relpath(_lib.LIB_PATH, ROOT), "device": mem.device_info(),
          "frames": frames, "warmup": warmup, "bandwidth_probe": probe, "scenes": {}}
ok = True
for name, meshes, instance_mesh, transforms in scenes():
    meshes = [m if len(m) == 3 else (m[0], m[1], m[1].shape[0]) for m in meshes]
    inst = list(range(len(meshes))) if instance_mesh is None else instance_mesh
    host_tris, _, bad = scene.assemble_tris([(v, f) if f is not None else (v, None, n) for v, f, n in meshes], inst, transforms)
    n = host_tris.shape[0]
    recs, keep = [], []
    nbytes = 48 * n + (48 * len(inst) if transforms is not None else 0)
    for v, f, nf in meshes:
        d_v = mem.upload(v); d_f = mem.upload(np.ascontiguousarray(f, np.int32)) if f is not None else 0
        keep += [d_v, d_f]
        recs.append((d_v, v.shape[0], d_f, nf, 4 * v.shape[1]))
    used = set(inst)
    nbytes += sum(v.nbytes for k, (v, f, nf) in enumerate(meshes) if k in used) + sum(12 * meshes[k][2] for k in inst if meshes[k][1] is not None)
    d_M = mem.upload(transforms) if transforms is not None else 0
    ms_scene = api.MeshScene(mem, recs, instance_mesh)
    assert ms_scene.num_tris == n and bad == 0
    d_tris = mem.alloc(48 * n)

    def assemble():
        ms_scene.assemble(d_M, d_tris)

    def upload():
        mem.free(mem.upload(host_tris))

    def assemble_build_grid():
        assemble()
        g = api.Grid(); api.build_grid(mem, d_tris, n, g, 0.12, 2.4); mem.synchronize()
        g.free()

    def to_first_ray():
        assemble()
        g = api.build_all(mem, d_tris, n); api.setup_traversal(g); mem.synchronize()
        g.free()

    assemble(); mem.synchronize()
    got = mem.download(d_tris, np.float32, 12 * n)
    assert got.tobytes() == host_tris.tobytes(), name + ": the assembled triangles are not the statement's"
    for _ in range(warmup):
        assemble(); upload(); assemble_build_grid()
    mem.synchronize()
    t_asm, t_up, t_ab, t_first = [], [], [], []
    for f in range(frames):
        t_asm.append(api.profile(assemble, mem))
        t0 = time.perf_counter(); upload(); t_up.append((time.perf_counter() - t0) * 1e3)
        if f % 4 == 0:
            t0 = time.perf_counter(); assemble_build_grid(); t_ab.append((time.perf_counter() - t0) * 1e3)
    row = {"triangles": n, "instances": len(inst), "meshes": len(meshes), "indexed": meshes[0][1] is not None, "transforms": transforms is not None,
           "assemble": stats(t_asm), "upload": stats(t_up), "assemble_build_grid": stats(t_ab), "compulsory_bytes": int(nbytes)}
    gbps = nbytes / (row["assemble"]["median_ms"] * 1e6)
    row["assemble_GBps"] = round(gbps, 1); row["share_of_copy_rate"] = round(gbps / probe["copy_GBps"], 3)
    row["upload_over_assemble"] = round(row["upload"]["median_ms"] / row["assemble"]["median_ms"], 1)
    row["assemble_faster_than_upload"] = bool(row["assemble"]["median_ms"] < row["upload"]["median_ms"])
    if name == "stadium_objects":
        to_first_ray()
        for _ in range(8):
            t0 = time.perf_counter(); to_first_ray(); t_first.append((time.perf_counter() - t0) * 1e3)
        row["new_vertices_to_first_ray"] = stats(t_first)
    if name != "dust":
        ok = ok and row["assemble_faster_than_upload"]
    result["scenes"][name] = row
    print(json.dumps({name: row}), flush=True)
    ms_scene.close()
    for p in keep + [d_M, d_tris]:
        mem.free(p)

result["condition_assemble_faster_than_upload_on_the_1M_scenes"] = ok
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(("OK" if ok else "FAILED") + ": assemble faster than upload on the 10^6-triangle scenes; written to " + os.path.relpath(out_path, ROOT))
mem.close()
sys.exit(0 if ok else 1)
