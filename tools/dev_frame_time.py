"""DEV TOOL: what a frame costs when it stays on the device (hagrid_render_frame, hagrid_amd/csrc/frame.hip) -- configuration 2's scene (soup-1M,
default parameters, camera of scene.camera), per image size, in ONE process, the variants alternating frame by frame after a warm-up, every frame
between its own pair of events on the context's stream:

  1. traverse      the traversal launch alone over a resident ray buffer
  2. frame_depth   hagrid_render_frame, depth mode: ray generation + traversal + shading, nothing crossing the bus
  3. host_path     the frame without the frame entry points: host rays uploaded (32 B per ray), traverse_grid, hits downloaded (16 B per ray); the host's
                   own ray generation and shading are NOT counted (in that path's favour)
  4. frame_ao4     hagrid_render_frame with four ambient-occlusion samples (five traversals, four of them any-hit)
  5. kernels       each new kernel alone (`--kernel-reps` launches between one pair of events), with bytes read + written / time next to the copy rate
                   hagrid_bandwidth_probe measures in the same run

One condition is checked: frame_depth is faster than host_path (the exit status says so); everything else is recorded.  Written to --out (default
profiles/frame_time.json) with build.source_hash().

usage: python tools/dev_frame_time.py [--sizes 1024,4096] [--frames 200] [--warmup 20] [--tris 1000000] [--kernel-reps 50] [--out profiles/frame_time.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import api, scene, build as _build

arg = lambda name, default: (sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default)
sizes = [int(v) for v in arg("--sizes", "1024,4096").split(",")]
frames = int(arg("--frames", "200")); warmup = int(arg("--warmup", "20")); reps = int(arg("--kernel-reps", "50"))
num_tris = int(arg("--tris", "1000000"))
out_path = arg("--out", os.path.join(ROOT, "profiles", "frame_time.json"))

mem = api.MemManager(keep=True)
tris = scene.make_soup(num_tris)
d_tris = mem.upload(tris)
grid = api.build_all(mem, d_tris, tris.shape[0]); api.setup_traversal(grid)
probe = mem.bandwidth_probe(1 << 30, 5)
result = {"tool": "tools/dev_frame_time.py", "source_hash": _build.source_hash(), "device": mem.device_info(), "scene": f"soup-{num_tris}", "grid": grid.summary(),
          "frames": frames, "warmup": warmup, "bandwidth_probe": probe, "sizes": {}}


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 5), "mean_ms": round(float(a.mean()), 5), "min_ms": round(float(a[0]), 5), "p90_ms": round(float(a[int(0.9 * (a.size - 1))]), 5)}


ok = True
for W in sizes:
    n = W * W
    cam = scene.camera(grid.bbox_min, grid.bbox_max)
    clip = float(cam[4]); radius = 0.1 * clip
    ws = mem.alloc(api.frame_workspace_bytes(W, W, 4)); lay = api.frame_workspace_layout(W, W, 4)
    d_px = mem.alloc(4 * n)
    d_rays = mem.alloc(32 * n); d_hits = mem.alloc(16 * n)                      # the resident buffer of variant 1 and the device side of variant 3
    api.gen_primary_rays(mem, cam, clip, W, W, d_rays)
    host_rays = mem.download(d_rays, np.float32, 8 * n).reshape(n, 8)            # the bits of scene.make_rays_primary (tests/test_frame_gpu.py)
    host_hits = np.empty(n, dtype=api.HIT_DTYPE)

    def traverse():
        api.traverse_grid(grid, d_tris, d_rays, d_hits, n)

    def frame_depth():
        api.render_frame(grid, d_tris, cam, clip, W, W, ws, d_px, mode=api.SHADE_DEPTH)

    def host_path():
        mem.copy_h2d(d_rays, host_rays)
        api.traverse_grid(grid, d_tris, d_rays, d_hits, n)
        mem.copy_d2h(host_hits, d_hits)

    def frame_ao4():
        api.render_frame(grid, d_tris, cam, clip, W, W, ws, d_px, ao_samples=4, ao_radius=radius, seed=1)

    variants = [("traverse", traverse), ("frame_depth", frame_depth), ("host_path", host_path), ("frame_ao4", frame_ao4)]
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    mem.synchronize()
    ms = {name: [] for name, _ in variants}; wall = {name: [] for name, _ in variants}
    for f in range(frames):
        for name, fn in variants:                                                # alternating: one frame of each, in turn
            t0 = time.perf_counter()
            ms[name].append(api.profile(fn, mem))                                # event pair; profile() returns when the second event is reached
            wall[name].append((time.perf_counter() - t0) * 1e3)
    row = {"rays": n, "events": {k: stats(v) for k, v in ms.items()}, "host_clock": {k: stats(v) for k, v in wall.items()}}
    ev = row["events"]
    row["frame_minus_traverse_ms"] = round(ev["frame_depth"]["median_ms"] - ev["traverse"]["median_ms"], 5)
    row["frame_depth_faster_than_host_path"] = bool(ev["frame_depth"]["median_ms"] < ev["host_path"]["median_ms"])
    row["host_path_over_frame_depth"] = round(ev["host_path"]["median_ms"] / ev["frame_depth"]["median_ms"], 2)
    ok = ok and row["frame_depth_faster_than_host_path"]

    # 5. the kernels alone; the hits of the last depth frame are in the workspace (rays at 0, primary hits behind them)
    frame_depth(); mem.synchronize()
    w_rays, w_hits, w_bounce, w_occ, w_counts = (ws + lay[k] for k in ("rays", "hits", "bounce_rays", "occlusion_hits", "counts"))
    n_hit = int((mem.download(w_hits, api.HIT_DTYPE, n)["id"] >= 0).sum())
    mem.zero(w_occ, 16 * n); mem.zero(w_counts, 4 * n)
    kernels = [
        ("primary_rays", lambda: api.gen_primary_rays(mem, cam, clip, W, W, w_rays), 32 * n),
        ("bounce_rays_inactive_misses", lambda: api.gen_bounce_rays(mem, d_tris, w_rays, w_hits, n, 1, grid.bbox_min, grid.bbox_max, w_bounce, tmax=radius, redraw_misses=False), 16 * n + (32 + 12) * n_hit + 32 * n),
        ("bounce_rays_redrawn_misses", lambda: api.gen_bounce_rays(mem, d_tris, w_rays, w_hits, n, 1, grid.bbox_min, grid.bbox_max, w_bounce), 16 * n + (32 + 12) * n_hit + 32 * n),
        ("shade_hits_depth", lambda: api.shade_hits(mem, w_hits, n, api.SHADE_DEPTH, clip, d_px), 20 * n),
        ("shade_hits_heat", lambda: api.shade_hits(mem, w_hits, n, api.SHADE_HEAT, clip, d_px), 20 * n),
        ("accumulate_occlusion", lambda: api.accumulate_occlusion(mem, w_occ, n, w_counts), 24 * n),
        ("shade_occlusion", lambda: api.shade_occlusion(mem, w_hits, w_counts, n, 4, d_px), 24 * n),
    ]
    row["kernels"] = {}
    for name, fn, nbytes in kernels:
        def burst():
            for _ in range(reps):
                fn()
        burst(); mem.synchronize()
        best = min(api.profile(burst, mem) for _ in range(5)) / reps
        gbps = nbytes / (best * 1e6)
        row["kernels"][name] = {"ms": round(best, 5), "bytes": int(nbytes), "GBps": round(gbps, 1), "share_of_copy_rate": round(gbps / probe["copy_GBps"], 3)}
    row["primary_hits"] = n_hit
    result["sizes"][str(W)] = row
    print(json.dumps({str(W): row}), flush=True)
    for p in (ws, d_px, d_rays, d_hits):
        mem.free(p)

result["condition_frame_depth_faster_than_host_path"] = ok
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(("OK" if ok else "FAILED") + ": frame_depth faster than host_path; written to " + os.path.relpath(out_path, ROOT))
mem.close()
sys.exit(0 if ok else 1)
