"""Frames on the device, the part that needs no GPU: the per-ray functions of include/hagrid/frame.h -- the arithmetic of the kernels in
hagrid_amd/csrc/frame.hip -- compiled for the host and compared BIT FOR BIT with the numpy statement in hagrid_amd/scene.py; the new
keyword arguments of scene.make_rays_bounce keep its old output; the new entry points are exported and the workspace layout is the
documented one."""
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def frame_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_host")
    exe = str(d / "frame_host")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC,
                    os.path.join(ROOT, "tests", "cpp", "frame_host.cpp"), "-o", exe], check=True)

    def run(op, params: bytes, inputs, out_dtype):
        names = []
        (d / "params.bin").write_bytes(params)
        for k, a in enumerate(inputs):
            f = str(d / f"in{k}.bin"); np.ascontiguousarray(a).tofile(f); names.append(f)
        out = str(d / "out.bin")
        subprocess.run([exe, op, str(d / "params.bin"), *names, out], check=True, timeout=300)
        return np.fromfile(out, dtype=out_dtype)

    return run


@pytest.fixture(scope="module")
def soup_case():
    """the smoke scene (20 000 triangles), 128 x 128 primary rays and the CPU oracle's hits for them"""
    import __graft_entry__ as g
    g.build()
    from hagrid_amd import scene
    from oracle import oracle as O
    tris = scene.make_soup(20000)
    G = O.Grid.full(tris)
    lo, hi = G.bbox_min, G.bbox_max
    rays = scene.make_rays_primary(lo, hi, 128, 128)
    hits, _ = G.traverse(tris, rays, nthreads=4)
    assert 0 < (hits["id"] >= 0).sum() < rays.shape[0]          # both rules (hit, miss) are exercised
    return tris, G, lo, hi, rays, hits


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _primary(frame_host, cam, w, h, first, count):
    eye, cdir, right, up, clip = cam
    params = struct.pack("<12f", *[float(v) for v in (*eye, *cdir, *right, *up)]) + struct.pack("<fiiqi", float(clip), w, h, first, count)
    return frame_host("primary", params, [], np.float32).reshape(-1, 8)


@pytest.mark.parametrize("w,h,kw", [(64, 64, {}), (333, 77, {}), (96, 40, {"yaw": 0.3, "strafe": 0.05}), (1, 1, {})])
def test_primary_rays_bit_identical_to_scene(frame_host, w, h, kw):
    from hagrid_amd import scene
    lo, hi = np.float32([0.0, -0.1, 0.05]), np.float32([1.0, 0.9, 1.2])
    cam = scene.camera(lo, hi, ratio=w / float(h), **kw)
    want = scene.make_rays_primary(lo, hi, w, h, **kw)
    got = _primary(frame_host, cam, w, h, 0, w * h)
    assert got.shape == want.shape and (bits(got) == bits(want)).all()


def test_primary_rays_slice(frame_host):
    from hagrid_amd import scene
    lo, hi = np.float32([0.0, 0.0, 0.0]), np.float32([1.0, 2.0, 1.5])
    w, h, first, count = 333, 77, 12345, 7001
    cam = scene.camera(lo, hi, ratio=w / float(h))
    want = scene.make_rays_primary(lo, hi, w, h, first=first, count=count)
    got = _primary(frame_host, cam, w, h, first, count)
    assert got.shape == (count, 8) and (bits(got) == bits(want)).all()


def _bounce(frame_host, tris, rays, hits, lo, hi, seed, first, tmax, redraw):
    params = struct.pack("<QQ3f3ffIi", seed, first, *[float(v) for v in lo], *[float(v) for v in hi], float(tmax), 1 if redraw else 0, rays.shape[0])
    return frame_host("bounce", params, [tris, rays, hits], np.float32).reshape(-1, 8)


@pytest.mark.parametrize("redraw", [True, False])
@pytest.mark.parametrize("seed,first", [(0x52415953 + 5, 0), (0xFEDCBA9876543210, (1 << 32) + 12345)])
def test_bounce_rays_bit_identical_to_scene(frame_host, soup_case, seed, first, redraw):
    from hagrid_amd import scene
    tris, G, lo, hi, rays, hits = soup_case
    tmax = 0.125 if not redraw else float(scene.FLT_MAX)
    want = scene.make_rays_bounce(tris, rays, hits, lo, hi, seed, first=first, tmax=tmax, redraw_misses=redraw)
    got = _bounce(frame_host, tris, rays, hits, lo, hi, seed, first, tmax, redraw)
    assert got.shape == want.shape
    diff = (bits(got) != bits(want)).any(axis=1)
    assert not diff.any(), f"{diff.sum()} of {diff.size} rays differ, first at {np.flatnonzero(diff)[:5]}"
    miss = hits["id"] < 0
    if not redraw:
        assert (want[miss] == np.float32([0, 0, 0, 0, 0, 0, 1, -1])).all() and (want[~miss, 7] == np.float32(tmax)).all()


def test_bounce_defaults_keep_the_parents_output():
    """scene.make_rays_bounce without the new keyword arguments: the sha256 of a small call, taken with the scene.py of the commit before them."""
    import __graft_entry__ as g
    g.build()
    from hagrid_amd import scene
    from oracle import oracle as O
    tris = scene.make_soup(2000)
    lo, hi = scene.tris_bbox(tris)
    rays = scene.make_rays_primary(lo, hi, 48, 32)
    hits, _ = O.Grid.full(tris).traverse(tris, rays, nthreads=2)
    assert hashlib.sha256(hits.tobytes()).hexdigest() == "7b460ae7b0dbd16d24dcdf9a97e71fb3c63e7e4c15d05d51a952c94a258db89e", "the oracle's hits moved, not the bounce rule"
    b = scene.make_rays_bounce(tris, rays, hits, lo, hi, 0x52415953 + 5, first=7)
    assert hashlib.sha256(b.tobytes()).hexdigest() == "278441f92221c507dc68b1b4f2ebf3046d7e337abf39c5c1c110cd66c1ba271c"


def test_inactive_rays_get_no_hit_from_the_oracle(soup_case):
    from hagrid_amd import scene
    tris, G, lo, hi, rays, hits = soup_case
    inactive = scene.make_rays_inactive(1000)
    oh, _ = G.traverse(tris, inactive, nthreads=1)
    assert (oh["id"] == -1).all() and (oh["t"] == np.float32(-1.0)).all()
    # ... and as the misses of a bounce batch
    b = scene.make_rays_bounce(tris, rays, hits, lo, hi, 3, tmax=0.1, redraw_misses=False)
    oh, _ = G.traverse(tris, b, nthreads=4)
    miss = hits["id"] < 0
    assert (oh["id"][miss] == -1).all() and (oh["t"][miss] == np.float32(-1.0)).all()


def _synthetic_hits():
    from hagrid_amd import scene
    ids = np.concatenate([np.arange(-1, 300), np.int32([1000, 70000, 2 ** 31 - 1])]).astype(np.int32)
    h = np.zeros(ids.size, dtype=scene.HIT_DTYPE)
    h["id"] = ids
    h["t"] = (np.arange(ids.size, dtype=np.float32) * np.float32(0.013)).astype(np.float32)
    return h


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_shade_hits_byte_identical_to_scene(frame_host, soup_case, mode):
    from hagrid_amd import scene
    tris, G, lo, hi, rays, hits = soup_case
    for h, clip in ((hits, float(rays[0, 7])), (_synthetic_hits(), 2.5), (_synthetic_hits(), 0.7)):
        want = scene.shade_hits(h, mode, clip)
        got = frame_host("shade", struct.pack("<ifi", mode, clip, h.shape[0]), [h], np.uint8).reshape(-1, 4)
        assert want.shape == got.shape and (got == want).all(), np.flatnonzero((got != want).any(axis=1))[:5]
        assert (want[:, 3] == 255).all()
        if mode != scene.SHADE_HEAT:
            assert (want[:, 0] == want[:, 1]).all() and (want[:, 1] == want[:, 2]).all()


def test_heat_gradient_end_points():
    from hagrid_amd import scene
    h = np.zeros(3, dtype=scene.HIT_DTYPE); h["id"] = [0, 40, 100]
    px = scene.shade_hits(h, scene.SHADE_HEAT)
    assert px[0].tolist() == [255, 0, 0, 255] and px[1].tolist() == [0, 128, 0, 255] and px[2, 0] == 0 and px[2, 2] >= 254     # blue, dark green, red


@pytest.mark.parametrize("samples", [1, 4, 7])
def test_shade_occlusion_byte_identical_to_scene(frame_host, soup_case, samples):
    from hagrid_amd import scene
    tris, G, lo, hi, rays, hits = soup_case
    counts = (np.arange(hits.shape[0]) % (samples + 1)).astype(np.int32)
    want = scene.shade_occlusion(hits, counts, samples)
    got = frame_host("ao", struct.pack("<ii", samples, hits.shape[0]), [hits, counts], np.uint8).reshape(-1, 4)
    assert (got == want).all()
    assert set(np.unique(want[:, 0]).tolist()) <= {255 * (samples - c) // samples for c in range(samples + 1)} | {0}
    assert (want[hits["id"] < 0, 0] == 0).all()


def test_frame_entry_points_exported_and_workspace_layout():
    import __graft_entry__ as g
    g.build()
    from hagrid_amd import api, lib
    L = lib.load()
    for name in ("hagrid_gen_primary_rays", "hagrid_gen_bounce_rays", "hagrid_shade_hits", "hagrid_accumulate_occlusion",
                 "hagrid_shade_occlusion", "hagrid_frame_workspace_bytes", "hagrid_render_frame"):
        assert name in lib.SIGNATURES and hasattr(L, name)
    for name in ("Camera", "gen_primary_rays", "gen_bounce_rays", "shade_hits", "accumulate_occlusion", "shade_occlusion",
                 "frame_workspace_bytes", "render_frame"):
        assert hasattr(api, name) and name in api.__all__
    import ctypes as C
    assert C.sizeof(lib.Camera) == 48
    up = lambda v: (v + 255) // 256 * 256
    for w, h in ((1, 1), (128, 128), (333, 77), (1024, 1024)):
        n = w * h
        assert api.frame_workspace_bytes(w, h, 0) == up(32 * n) + up(16 * n) == api.frame_workspace_layout(w, h, 0)["total"]
        assert api.frame_workspace_bytes(w, h, 4) == 2 * (up(32 * n) + up(16 * n)) + up(4 * n) == api.frame_workspace_layout(w, h, 4)["total"]
        lay = api.frame_workspace_layout(w, h, 4)
        assert lay["rays"] == 0 and lay["hits"] == up(32 * n) and all(v % 256 == 0 for v in lay.values())
    assert api.frame_workspace_bytes(0, 5, 0) == 0 and api.frame_workspace_bytes(5, -1, 0) == 0


def test_frame_header_is_cxx11_and_stays_out_of_the_other_headers():
    """include/hagrid/frame.h compiles as plain C++11, and no other header pulls it in (a program written against the reference declares its
    own global Camera / gen_camera / gen_rays next to `using namespace hagrid`)."""
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-DHOST=", "-DDEVICE=", "-I", INC, "-fsyntax-only", "-x", "c++",
                        os.path.join(INC, "hagrid", "frame.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in os.listdir(os.path.join(INC, "hagrid")) + ["../hagrid_amd.h"]:
        if name != "frame.h":
            assert not re.search(r'#\s*include\s*[<"][^>"]*frame\.h', open(os.path.join(INC, "hagrid", name)).read()), name
