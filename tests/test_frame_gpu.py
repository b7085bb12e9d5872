"""Frames on the device (hagrid_amd/csrc/frame.hip) on the GPU: every generator and shader against the numpy statement in hagrid_amd/scene.py
bit for bit, hagrid_render_frame against the CPU oracle's hits (pixels AND the hits left in the workspace), ambient occlusion against the
oracle's nearest-hit traversal of the same bounce rays, the reference viewer's heat map from step counts, a torch tensor as the pixel
buffer on torch's stream, bad arguments, and the front-end's --display / --ppm / --ao options."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _subproc
from _poison import alloc_out, assert_all_written, fetch
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def case():
    """the smoke scene: 20 000 triangles, grid built on the device, the CPU oracle's grid next to it"""
    from hagrid_amd import api
    from oracle import oracle as O
    tris = scene.make_soup(20000)
    mem = api.MemManager(keep=True)
    d_tris = mem.upload(tris)
    grid = api.build_all(mem, d_tris, tris.shape[0])
    api.setup_traversal(grid)

    class Case: pass
    c = Case()
    c.api, c.mem, c.tris, c.d_tris, c.grid, c.G = api, mem, tris, d_tris, grid, O.Grid.full(tris)
    c.lo, c.hi = grid.bbox_min, grid.bbox_max
    c.oracle_hits = {}

    def oracle(w, h, **kw):
        key = (w, h, tuple(sorted(kw.items())))
        if key not in c.oracle_hits:
            rays = scene.make_rays_primary(c.lo, c.hi, w, h, **kw)
            c.oracle_hits[key] = (rays, c.G.traverse(tris, rays, nthreads=8)[0])
        return c.oracle_hits[key]
    c.oracle = oracle
    yield c
    mem.close()


def render(c, w, h, mode=0, ao=0, radius=0.0, seed=0, ws=None, **kw):
    """one frame through hagrid_render_frame; returns (pixels (n, 4) uint8, rays, hits of the workspace)"""
    api, mem = c.api, c.mem
    cam = scene.camera(c.lo, c.hi, ratio=w / float(h), **kw)
    n = w * h
    own = ws is None
    if own:
        ws = mem.alloc(api.frame_workspace_bytes(w, h, ao))
    mem.one(ws, api.frame_workspace_bytes(w, h, ao))          # (rays and hits of the workspace are compared: not the previous frame's)
    d_px = alloc_out(mem, 4 * n)
    api.render_frame(c.grid, c.d_tris, cam, cam[4], w, h, ws, d_px, mode=mode, ao_samples=ao, ao_radius=radius, seed=seed)
    px = fetch(mem, d_px, np.uint8, 4 * n).reshape(n, 4)
    lay = api.frame_workspace_layout(w, h, ao)
    rays = mem.download(ws + lay["rays"], np.float32, 8 * n).reshape(n, 8)
    hits = mem.download(ws + lay["hits"], api.HIT_DTYPE, n)
    mem.free(d_px)
    if own:
        mem.free(ws)
    return px, rays, hits


@pytest.mark.parametrize("w,h,first,count,kw", [(333, 77, 0, None, {}), (1, 1, 0, None, {}), (130, 50, 4097, 1001, {"yaw": 0.2, "strafe": 0.03}), (64, 64, 0, None, {})])
def test_gen_primary_rays_bit_identical(case, w, h, first, count, kw):
    c = case; api, mem = c.api, c.mem
    cam = scene.camera(c.lo, c.hi, ratio=w / float(h), **kw)
    want = scene.make_rays_primary(c.lo, c.hi, w, h, first=first, count=count, **kw)
    n = want.shape[0]
    d = mem.alloc(32 * n + 32)
    mem.one(d, 32 * n + 32)
    api.gen_primary_rays(mem, cam, cam[4], w, h, d, first=first, count=count)
    got = mem.download(d, np.float32, 8 * n + 8)
    mem.free(d)
    assert (bits(got[:8 * n].reshape(n, 8)) == bits(want)).all()
    assert (got[8 * n:].view(np.uint32) == 0xFFFFFFFF).all(), "written beyond the range"


@pytest.mark.parametrize("redraw", [True, False])
@pytest.mark.parametrize("w,h,seed,first", [(128, 128, 0x52415953 + 5, 0), (333, 77, 0xFEDCBA9876543210, (1 << 32) + 12345)])
def test_gen_bounce_rays_bit_identical(case, w, h, seed, first, redraw):
    c = case; api, mem = c.api, c.mem
    rays, hits = c.oracle(w, h)
    n = rays.shape[0]
    tmax = 0.125 if not redraw else float(scene.FLT_MAX)
    want = scene.make_rays_bounce(c.tris, rays, hits, c.lo, c.hi, seed, first=first, tmax=tmax, redraw_misses=redraw)
    d_rays = mem.upload(rays); d_hits = mem.upload(hits); d_out = alloc_out(mem, 32 * n)
    api.gen_bounce_rays(mem, c.d_tris, d_rays, d_hits, n, seed, c.lo, c.hi, d_out, first=first, tmax=tmax, redraw_misses=redraw)
    got = fetch(mem, d_out, np.float32, 8 * n).reshape(n, 8)
    for p in (d_rays, d_hits, d_out):
        mem.free(p)
    diff = (bits(got) != bits(want)).any(axis=1)
    assert not diff.any(), f"{diff.sum()} of {n} rays differ, first at {np.flatnonzero(diff)[:5]}"


def _synthetic_hits(n):
    m = max(n, 4)
    h = np.zeros(m, dtype=scene.HIT_DTYPE)
    h["id"] = (np.arange(m) % 331 - 1).astype(np.int32)
    h["id"][-3:] = [1000, 70000, 2 ** 31 - 1]
    h["t"] = (np.arange(m, dtype=np.float32) * np.float32(0.0013)).astype(np.float32)
    return np.ascontiguousarray(h[m - n:])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 63, 1000, 257 * 3 + 5])
def test_shade_hits_byte_identical(case, mode, n):
    c = case; api, mem = c.api, c.mem
    h = _synthetic_hits(n)
    d_h = mem.upload(h); d_px = mem.alloc(4 * n + 4); mem.zero(d_px, 4 * n + 4)
    api.shade_hits(mem, d_h, n, mode, 0.9, d_px)
    got = mem.download(d_px, np.uint8, 4 * n + 4)
    mem.free(d_h); mem.free(d_px)
    assert (got[:4 * n].reshape(n, 4) == scene.shade_hits(h, mode, 0.9)).all() and (got[4 * n:] == 0).all()


@pytest.mark.parametrize("n,samples", [(1, 1), (1000, 4), (257 * 3 + 5, 7)])
def test_occlusion_accumulate_and_shade(case, n, samples):
    c = case; api, mem = c.api, c.mem
    prim = _synthetic_hits(n)
    d_prim = mem.upload(prim); d_counts = mem.alloc(4 * n + 4); mem.zero(d_counts, 4 * n + 4); d_px = alloc_out(mem, 4 * n)
    counts = np.zeros(n, np.int32)
    for s in range(samples):
        occ = np.zeros(n, dtype=scene.HIT_DTYPE)
        occ["id"] = np.where((np.arange(n) * 7 + s * 3) % 5 < 2, 17, -1)
        counts += occ["id"] >= 0
        d_occ = mem.upload(occ)
        api.accumulate_occlusion(mem, d_occ, n, d_counts)
        mem.synchronize(); mem.free(d_occ)
    got_counts = mem.download(d_counts, np.int32, n + 1)
    assert (got_counts[:n] == counts).all() and got_counts[n] == 0
    api.shade_occlusion(mem, d_prim, d_counts, n, samples, d_px)
    got = fetch(mem, d_px, np.uint8, 4 * n).reshape(n, 4)
    for p in (d_prim, d_counts, d_px):
        mem.free(p)
    assert (got == scene.shade_occlusion(prim, counts, samples)).all()


@pytest.mark.parametrize("w,h", [(128, 128), (333, 77)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_render_frame_matches_the_oracle(case, w, h, mode):
    c = case
    want_rays, oh = c.oracle(w, h)
    px, rays, hits = render(c, w, h, mode=mode)
    assert (bits(rays) == bits(want_rays)).all()
    assert (hits["id"] == oh["id"]).all() and (bits(hits["t"]) == bits(oh["t"])).all(), "the hits in the workspace are not the oracle's"
    assert (px == scene.shade_hits(oh, mode, float(want_rays[0, 7]))).all()
    assert 0 < (oh["id"] >= 0).sum() < w * h


@pytest.mark.parametrize("w,h", [(128, 128), (333, 77)])
def test_render_frame_ambient_occlusion_matches_the_oracle(case, w, h):
    c = case
    prim_rays, oh = c.oracle(w, h)
    samples, seed = 4, 0xA0
    radius = 0.1 * float(prim_rays[0, 7])
    counts = np.zeros(w * h, np.int64)
    for s in range(samples):
        b = scene.make_rays_bounce(c.tris, prim_rays, oh, c.lo, c.hi, seed + s, first=0, tmax=radius, redraw_misses=False)
        counts += c.G.traverse(c.tris, b, nthreads=8)[0]["id"] >= 0
    want = scene.shade_occlusion(oh, counts, samples)
    px, rays, hits = render(c, w, h, ao=samples, radius=radius, seed=seed)
    assert (hits["id"] == oh["id"]).all()
    assert (px == want).all(), f"{(px != want).any(axis=1).sum()} of {w * h} pixels differ"
    assert len(np.unique(want[:, 0])) >= 3          # occluded, partly occluded and open pixels all occur
    # the counts the frame left in its workspace
    lay = c.api.frame_workspace_layout(w, h, samples)
    assert lay["total"] == c.api.frame_workspace_bytes(w, h, samples)


def test_heat_map_of_step_counts_is_the_reference_viewers_picture(case):
    c = case; api, mem = c.api, c.mem
    w, h = 128, 128
    n = w * h
    ws = mem.alloc(api.frame_workspace_bytes(w, h, 0))
    mem.set_option("traverse.id_is_steps", 1)
    try:
        px, rays, hits = render(c, w, h, mode=api.SHADE_HEAT, ws=ws)
        with pytest.raises(api.HagridError):       # ambient occlusion needs primitive ids
            render(c, w, h, ao=2, radius=0.1)
    finally:
        mem.set_option("traverse.id_is_steps", 0)
    d_steps = alloc_out(mem, 4 * n); d_hits = alloc_out(mem, 16 * n)
    api.traverse_grid_stats(c.grid, c.d_tris, ws, d_hits, n, d_steps)
    steps = fetch(mem, d_steps, np.int32, n)
    assert_all_written(fetch(mem, d_hits, c.api.HIT_DTYPE, n))
    for p in (d_steps, d_hits, ws):
        mem.free(p)
    assert (hits["id"] == steps).all()
    as_hits = np.zeros(n, dtype=scene.HIT_DTYPE); as_hits["id"] = steps
    assert (px == scene.shade_hits(as_hits, scene.SHADE_HEAT)).all()
    assert len(np.unique(px[:, :3], axis=0)) > 4


def test_two_cameras_through_one_workspace(case):
    """the traversal remembers ray buffers by address (row length, tile order): a second camera's rays in the same buffer must not meet the first one's hints"""
    c = case; api, mem = c.api, c.mem
    w, h = 128, 128
    ws = mem.alloc(api.frame_workspace_bytes(w, h, 0))
    for rounds in range(3):
        for kw in ({}, {"yaw": 0.35, "strafe": 0.1}):
            want_rays, oh = c.oracle(w, h, **kw)
            px, rays, hits = render(c, w, h, mode=api.SHADE_DEPTH, ws=ws, **kw)
            assert (hits["id"] == oh["id"]).all() and (bits(hits["t"]) == bits(oh["t"])).all()
            assert (px == scene.shade_hits(oh, scene.SHADE_DEPTH, float(want_rays[0, 7]))).all()
    mem.free(ws)


def test_frame_into_a_torch_tensor_on_torchs_stream(case):
    import torch
    c = case; api, mem = c.api, c.mem
    w, h = 333, 77
    want_rays, oh = c.oracle(w, h)
    cam = scene.camera(c.lo, c.hi, ratio=w / float(h))
    ws = mem.alloc(api.frame_workspace_bytes(w, h, 0))
    mem.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        mem.use_stream(torch.cuda.current_stream().cuda_stream)
        try:
            api.render_frame(c.grid, c.d_tris, cam, cam[4], w, h, ws, img.data_ptr(), mode=api.SHADE_DEPTH)
            bgr_sum = img[..., :3].to(torch.int32).sum(dim=-1)       # torch work queued behind the frame on the same stream
        finally:
            stream.synchronize()
            mem.use_stream(None)
    want = scene.shade_hits(oh, scene.SHADE_DEPTH, float(want_rays[0, 7])).reshape(h, w, 4)
    assert (img.cpu().numpy() == want).all()
    assert (bgr_sum.cpu().numpy() == want[..., :3].astype(np.int32).sum(axis=-1)).all()
    mem.free(ws)


def test_bad_arguments_are_einval_and_the_context_stays_usable(case):
    c = case; api, mem = c.api, c.mem
    L, ctx, E = mem._L, mem._ctx, -1
    cam = api.Camera.from_scene(scene.camera(c.lo, c.hi))
    w = h = 16
    n = w * h
    ws = mem.alloc(api.frame_workspace_bytes(w, h, 2)); d_px = mem.alloc(4 * n)
    vp = C.c_void_p
    f3 = (C.c_float * 3)(0, 0, 0)
    assert L.hagrid_gen_primary_rays(ctx, None, 1.0, w, h, 0, n, vp(ws)) == E
    assert L.hagrid_gen_primary_rays(ctx, C.byref(cam), 1.0, w, h, 0, n, None) == E
    assert L.hagrid_gen_primary_rays(ctx, C.byref(cam), 1.0, 0, h, 0, n, vp(ws)) == E
    assert L.hagrid_gen_primary_rays(ctx, C.byref(cam), 1.0, w, -1, 0, n, vp(ws)) == E
    assert L.hagrid_gen_primary_rays(ctx, C.byref(cam), 1.0, w, h, 0, 0, vp(ws)) == E
    assert L.hagrid_gen_primary_rays(ctx, C.byref(cam), 1.0, w, h, 1, n, vp(ws)) == E          # one pixel beyond the image
    assert L.hagrid_gen_primary_rays(ctx, C.byref(cam), 1.0, w, h, -1, 4, vp(ws)) == E
    assert b"pixel range" in L.hagrid_last_error(ctx)
    assert L.hagrid_gen_bounce_rays(ctx, vp(c.d_tris), vp(ws), vp(ws + 32 * n), n, 1, 0, f3, f3, 1.0, 0, vp(ws)) == E      # out == in
    assert L.hagrid_gen_bounce_rays(ctx, None, vp(ws), vp(ws + 32 * n), n, 1, 0, f3, f3, 1.0, 0, vp(d_px)) == E
    assert L.hagrid_gen_bounce_rays(ctx, vp(c.d_tris), vp(ws), vp(ws + 32 * n), 0, 1, 0, f3, f3, 1.0, 0, vp(d_px)) == E
    assert L.hagrid_gen_bounce_rays(ctx, vp(c.d_tris), vp(ws), vp(ws + 32 * n), n, 1, 0, f3, f3, 1.0, 8, vp(d_px)) == E    # unknown flag
    assert L.hagrid_shade_hits(ctx, vp(ws), n, 3, 1.0, vp(d_px)) == E
    assert L.hagrid_shade_hits(ctx, vp(ws), n, -1, 1.0, vp(d_px)) == E
    assert L.hagrid_shade_hits(ctx, vp(ws), n, 0, 0.0, vp(d_px)) == E                             # depth needs clip > 0
    assert L.hagrid_shade_hits(ctx, vp(ws), 0, 0, 1.0, vp(d_px)) == E
    assert L.hagrid_shade_hits(ctx, None, n, 0, 1.0, vp(d_px)) == E
    assert L.hagrid_accumulate_occlusion(ctx, vp(ws), n, None) == E
    assert L.hagrid_accumulate_occlusion(ctx, vp(ws), -5, vp(d_px)) == E
    assert L.hagrid_shade_occlusion(ctx, vp(ws), vp(d_px), n, 0, vp(d_px)) == E
    assert L.hagrid_shade_occlusion(ctx, vp(ws), None, n, 2, vp(d_px)) == E
    g = C.byref(c.grid.pod)
    assert L.hagrid_render_frame(ctx, g, vp(c.d_tris), C.byref(cam), 1.0, w, h, 7, 0, 0.0, 0, vp(ws), vp(d_px)) == E
    assert L.hagrid_render_frame(ctx, g, vp(c.d_tris), C.byref(cam), 0.0, w, h, 0, 0, 0.0, 0, vp(ws), vp(d_px)) == E
    assert L.hagrid_render_frame(ctx, g, vp(c.d_tris), C.byref(cam), 1.0, w, 0, 0, 0, 0.0, 0, vp(ws), vp(d_px)) == E
    assert L.hagrid_render_frame(ctx, g, vp(c.d_tris), C.byref(cam), 1.0, w, h, 0, -1, 0.0, 0, vp(ws), vp(d_px)) == E
    assert L.hagrid_render_frame(ctx, g, vp(c.d_tris), C.byref(cam), 1.0, w, h, 0, 0, 0.0, 0, None, vp(d_px)) == E
    assert L.hagrid_render_frame(ctx, None, vp(c.d_tris), C.byref(cam), 1.0, w, h, 0, 0, 0.0, 0, vp(ws), vp(d_px)) == E
    assert L.hagrid_frame_workspace_bytes(0, 4, 0) == 0
    with pytest.raises(api.HagridError):
        api.shade_hits(mem, ws, n, 9, 1.0, d_px)
    mem.free(ws); mem.free(d_px)
    # the context still renders
    want_rays, oh = c.oracle(128, 128)
    px, rays, hits = render(c, 128, 128, mode=0)
    assert (hits["id"] == oh["id"]).all() and (px == scene.shade_hits(oh, 0, float(want_rays[0, 7]))).all()


@pytest.fixture(scope="module")
def cli():
    import torch
    hip_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "hagrid_cli")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC, os.path.join(ROOT, "tools", "hagrid_cli.cpp"),
                        "-o", exe, "-L", os.path.join(ROOT, "hagrid_amd"), "-lhagrid_amd", "-L", hip_lib, "-lamdhip64", "-ldl",
                        "-Wl,-rpath," + os.path.join(ROOT, "hagrid_amd"), "-Wl,-rpath," + hip_lib, "-Wl,--allow-shlib-undefined"], check=True)
        yield exe, d


def _read_pnm(path, magic, channels):
    data = open(path, "rb").read()
    m = re.match(rb"(P\d)\n(\d+) (\d+)\n255\n", data)
    assert m and m.group(1) == magic
    w, h = int(m.group(2)), int(m.group(3))
    body = np.frombuffer(data[m.end():], dtype=np.uint8)
    assert body.size == w * h * channels
    return body.reshape(h * w, channels), w, h


def test_cli_depth_frame_pgm_and_ppm_agree(cli):
    """-o is shaded on the host (a miss is 255 by id), --ppm by the device kernel (the reference's formula: a miss is 255 * clip / clip = 254 or 255)"""
    exe, d = cli
    pgm, ppm = os.path.join(d, "f.pgm"), os.path.join(d, "f.ppm")
    r = _subproc.check([exe, "soup:20000", "-sx", "256", "-sy", "128", "-o", pgm, "--ppm", ppm, "--display", "depth"])
    m = re.search(r"(\d+) intersection\(s\)", r.stdout)
    assert m, r.stdout
    gray, w, h = _read_pnm(pgm, b"P5", 1)
    rgb, w2, h2 = _read_pnm(ppm, b"P6", 3)
    assert (w, h) == (w2, h2) == (256, 128)
    assert (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 1] == rgb[:, 2]).all()
    below = gray[:, 0] < 255
    assert (rgb[below, 0] == gray[below, 0]).all()
    assert np.isin(rgb[~below, 0], [254, 255]).all()
    assert 0 < below.sum() <= int(m.group(1))


def test_cli_ambient_occlusion_ppm(cli):
    exe, d = cli
    ppm = os.path.join(d, "ao.ppm")
    r = _subproc.check([exe, "soup:20000", "-sx", "200", "-sy", "100", "--ao", "4", "--ppm", ppm])
    rgb, w, h = _read_pnm(ppm, b"P6", 3)
    assert (w, h) == (200, 100), r.stdout
    assert np.isin(rgb, [255 * (4 - k) // 4 for k in range(5)] + [0]).all()
    assert (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 1] == rgb[:, 2]).all() and len(np.unique(rgb)) >= 3


def test_cli_heat_display_ppm(cli):
    """--display heat colours by traversal step count, the reference viewer's picture: the gradient's colours, not a grey ramp"""
    exe, d = cli
    ppm = os.path.join(d, "heat.ppm")
    _subproc.check([exe, "soup:20000", "-sx", "160", "-sy", "96", "--display", "heat", "--ppm", ppm])
    rgb, w, h = _read_pnm(ppm, b"P6", 3)
    assert (w, h) == (160, 96)
    steps = np.arange(0, 101)
    as_hits = np.zeros(steps.size, dtype=scene.HIT_DTYPE); as_hits["id"] = steps
    palette = {tuple(int(v) for v in px[[2, 1, 0]]) for px in scene.shade_hits(as_hits, scene.SHADE_HEAT)}       # B G R A -> R G B
    seen = {tuple(int(v) for v in c) for c in np.unique(rgb, axis=0)}
    assert seen <= palette and len(seen) > 4
