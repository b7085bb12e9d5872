"""The C++ API mirror (include/hagrid/*.h): compiles as plain C++ the way the reference compiles main.cpp, and -- on the GPU -- a C++
program driving build/merge/flatten/expand/compress/traverse through the headers matches a host brute force."""
import os
import subprocess
import sys
import tempfile

import pytest

import _poison
import _subproc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_headers_compile_as_plain_cxx():
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-DHOST=", "-DDEVICE=", "-I", INC, "-fsyntax-only",
                        os.path.join(ROOT, "tests", "cpp", "api_drop_in.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_l0_host_functions_match_golden(golden_dir):
    """The HOST instantiation of the product's L0 headers against the reference-header golden vectors."""
    import numpy as np
    src = r'''
#include <cstdio>
#include "hagrid/grid.h"
#include "hagrid/prims.h"
using namespace hagrid;
extern "C" {
int p_ipr(const Tri* t, const Ray* r, int id, Hit* h) { return intersect_prim_ray(*t, *r, id, *h); }
int p_ipc(const Tri* t, const BBox* b) { return intersect_prim_cell(*t, *b); }
void p_range(const int* d, const BBox* g, const BBox* o, int* out) { Range r = compute_range(ivec3(d[0], d[1], d[2]), *g, *o); out[0]=r.lx; out[1]=r.ly; out[2]=r.lz; out[3]=r.hx; out[4]=r.hy; out[5]=r.hz; }
void p_dims(const BBox* b, int n, float dens, int* out) { ivec3 d = compute_grid_dims(*b, n, dens); out[0]=d.x; out[1]=d.y; out[2]=d.z; }
unsigned p_lookup(const Entry* e, int shift, const int* td, const int* v) { return lookup_entry(e, shift, ivec3(td[0], td[1], td[2]), ivec3(v[0], v[1], v[2])); }
int p_ilog2(int t) { return ilog2(t); }
float p_rcp(float x) { return safe_rcp(x); }
float p_prodsign(float x, float y) { return prodsign(x, y); }
unsigned p_entry(unsigned a, unsigned b) { return as<unsigned>(make_entry(a, b)); }
}
'''
    import ctypes as C
    kat = np.load(os.path.join(golden_dir, "l0_kat.npz"))
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "p.cpp"); open(f, "w").write(src)
        so = os.path.join(d, "p.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-DHOST=", "-DDEVICE=", "-I", INC, f, "-o", so], check=True)
        L = C.CDLL(so)
        L.p_rcp.restype = C.c_float; L.p_rcp.argtypes = [C.c_float]
        L.p_prodsign.restype = C.c_float; L.p_prodsign.argtypes = [C.c_float, C.c_float]
        L.p_lookup.restype = C.c_uint; L.p_entry.restype = C.c_uint
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        bits = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)
        assert (bits([L.p_rcp(float(v)) for v in kat["rcp_in"]]) == bits(kat["rcp_out"])).all()
        assert (bits([L.p_prodsign(float(a), float(b)) for a, b in zip(kat["prodsign_x"], kat["prodsign_y"])]) == bits(kat["prodsign_out"])).all()
        assert [L.p_ilog2(int(v)) for v in kat["ilog2_in"]] == list(kat["ilog2_out"])
        assert [L.p_entry(int(a), int(b)) for a, b in zip(kat["entry_log_dim"], kat["entry_begin"])] == list(kat["entry_out"])
        tris = np.ascontiguousarray(kat["tris"])
        rays, tid = np.ascontiguousarray(kat["ipr_rays"]), kat["ipr_tid"]
        hit_dt = np.dtype([("id", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])
        for i in range(0, rays.shape[0], 3):
            h = np.array([(-1, rays[i, 7], 0, 0)], dtype=hit_dt)
            ret = L.p_ipr(p(tris[tid[i]:tid[i] + 1]), p(rays[i:i + 1]), int(tid[i]), p(h))
            assert ret == kat["ipr_ret"][i] and h["id"][0] == kat["ipr_hit_id"][i] and bits(h["t"])[0] == bits(kat["ipr_hit_t"][i:i + 1])[0]
        boxes, tid = np.ascontiguousarray(kat["ipc_boxes"]), kat["ipc_tid"]
        for i in range(0, boxes.shape[0], 3):
            assert L.p_ipc(p(tris[tid[i]:tid[i] + 1]), p(boxes[i:i + 1])) == kat["ipc_ret"][i]
        out = np.zeros(6, np.int32)
        a, b, c = (np.ascontiguousarray(kat[k]) for k in ("range_dims", "range_grid_bb", "range_obj_bb"))
        for i in range(0, a.shape[0], 2):
            L.p_range(p(a[i:i + 1]), p(b[i:i + 1]), p(c[i:i + 1]), p(out)); assert (out == kat["range_out"][i]).all()
        out = np.zeros(3, np.int32)
        a, b, c = (np.ascontiguousarray(kat[k]) for k in ("gd_bb", "gd_nprims", "gd_density"))
        for i in range(0, a.shape[0], 2):
            L.p_dims(p(a[i:i + 1]), int(b[i]), C.c_float(float(c[i])), p(out)); assert (out == kat["gd_out"][i]).all()
        for tag in ("octree", "flat"):
            ent = np.ascontiguousarray(kat[f"lk_{tag}_entries"]); vox = np.ascontiguousarray(kat[f"lk_{tag}_voxels"]); td = np.ascontiguousarray(kat[f"lk_{tag}_dims"])
            for i in range(0, vox.shape[0], 5):
                assert L.p_lookup(p(ent), int(kat[f"lk_{tag}_shift"]), p(td), p(vox[i:i + 1])) == kat[f"lk_{tag}_out"][i]


@pytest.mark.gpu
def test_cpp_program_through_the_headers_on_gpu():
    import torch
    hip_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drop_in")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC, os.path.join(ROOT, "tests", "cpp", "api_drop_in.cpp"),
                        "-o", exe, "-L", os.path.join(ROOT, "hagrid_amd"), "-lhagrid_amd", "-L", hip_lib, "-lamdhip64",
                        "-Wl,-rpath," + os.path.join(ROOT, "hagrid_amd"), "-Wl,-rpath," + hip_lib, "-Wl,--allow-shlib-undefined"], check=True)
        r = _subproc.check([exe, "20000", "4096"], timeout=120)
        sys.stdout.write(r.stdout)
        assert " 0 mismatches vs host" in r.stdout and "\n0 mismatches in the any-hit" in r.stdout, r.stdout


def _build_cli(d, hip_lib=None):
    if hip_lib is None:
        import torch
        hip_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    exe = os.path.join(d, "hagrid_cli")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC, os.path.join(ROOT, "tools", "hagrid_cli.cpp"),
                    "-o", exe, "-L", os.path.join(ROOT, "hagrid_amd"), "-lhagrid_amd", "-L", hip_lib, "-lamdhip64", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "hagrid_amd"), "-Wl,-rpath," + hip_lib, "-Wl,--allow-shlib-undefined"], check=True)
    return exe


def test_cli_usage_and_option_errors_need_no_gpu():
    with tempfile.TemporaryDirectory() as d:
        exe = _build_cli(d)
        r = subprocess.run([exe, "--help"], capture_output=True, text=True)
        assert r.returncode == 0 and "--top-density" in r.stdout and "--ray-file" in r.stdout and "--compress" in r.stdout and "--any-hit" in r.stdout
        r = subprocess.run([exe, "--bogus", "x.obj"], capture_output=True, text=True)
        assert r.returncode == 1 and "Unknown argument: --bogus" in r.stderr
        r = subprocess.run([exe, "-td"], capture_output=True, text=True)
        assert r.returncode == 1 and "Argument missing for: -td" in r.stderr
        r = subprocess.run([exe, "-k"], capture_output=True, text=True)
        assert r.returncode == 1 and "No model specified" in r.stderr


@pytest.fixture(scope="module")
def cli_case():
    """hagrid_cli built once, an OBJ scene (absolute, v/vt/vn and negative index forms mixed), a .rays file, and the number of
    intersections the Python API finds for them.  The parent keeps its context alive while the CLI runs, as a renderer's
    host process would."""
    import numpy as np
    from hagrid_amd import api, scene
    tris = scene.make_soup(5000)
    v0 = tris[:, 0:3]; v1 = v0 - tris[:, 4:7]; v2 = v0 + tris[:, 8:11]
    with tempfile.TemporaryDirectory() as d:
        exe = _build_cli(d)
        obj = os.path.join(d, "soup.obj")
        with open(obj, "w") as f:
            f.write("# soup\n")
            for a, b, c in zip(v0, v1, v2):
                for p in (a, b, c):
                    f.write("v %r %r %r\n" % (float(p[0]), float(p[1]), float(p[2])))
            for i in range(tris.shape[0]):
                if i % 3 == 0: f.write(f"f {3*i+1} {3*i+2} {3*i+3}\n")
                elif i % 3 == 1: f.write(f"f {3*i+1}/1/1 {3*i+2}/1/1 {3*i+3}/1/1\n")
                else: f.write(f"f {3*i+1-3*5000-1} {3*i+2-3*5000-1} {3*i+3-3*5000-1}\n")
        mem = api.MemManager(keep=True)
        # the OBJ round trip re-derives e1, e2, n from printed vertices: build the reference result from the same vertices
        t2 = scene.tris_from_vertices(v0, v1.astype(np.float32), v2.astype(np.float32))
        d_tris = mem.upload(t2)
        grid = api.build_all(mem, d_tris, t2.shape[0])
        rays = scene.make_rays_incoherent(grid.bbox_min, grid.bbox_max, 50000, 5)
        rays[:, 3] = 0.0; rays[:, 7] = scene.FLT_MAX
        rfile = os.path.join(d, "soup.rays")
        np.ascontiguousarray(rays[:, [0, 1, 2, 4, 5, 6]]).tofile(rfile)
        d_rays = mem.upload(rays); d_hits = _poison.alloc_out(mem, 16 * rays.shape[0])
        api.traverse_grid(grid, d_tris, d_rays, d_hits, rays.shape[0])
        hits = _poison.fetch(mem, d_hits, api.HIT_DTYPE, rays.shape[0])
        _poison.assert_all_written(hits)                  # (only the count of hits is compared: a ray the launch skipped would read as a miss)
        want = int((hits["id"] >= 0).sum())

        class Case: pass
        c = Case()
        c.dir, c.exe, c.obj, c.rays, c.want, c.cells, c.refs = d, exe, obj, rfile, want, grid.num_cells, grid.num_refs
        yield c
        mem.close()


@pytest.mark.gpu
def test_cli_obj_scene_and_ray_file_benchmark(cli_case):
    """OBJ scene + .rays file through the CLI; the intersection count equals the Python API's."""
    c = cli_case
    r = _subproc.check([c.exe, c.obj, "-r", c.rays, "-n", "3", "-w", "1", "-k", "-nb", "2"])
    assert "5000 triangle(s)" in r.stdout and "Grid built in " in r.stdout and "Entering benchmark mode" in r.stdout
    assert f"{c.cells} cells, {c.refs} references)" in r.stdout
    assert f"{c.want} intersection(s)." in r.stdout and " Mrays/sec." in r.stdout and "# Median: " in r.stdout


@pytest.mark.gpu
def test_cli_synthetic_scene_compressed_frame_image(cli_case):
    c = cli_case
    img = os.path.join(c.dir, "frame.pgm")
    r = _subproc.check([c.exe, "soup:20000", "-z", "-sx", "256", "-sy", "128", "-o", img])
    assert "20000 triangle(s)" in r.stdout and "Tracing one 256x128 frame" in r.stdout
    assert os.path.getsize(img) == len("P5\n256 128\n255\n") + 256 * 128


@pytest.mark.gpu
def test_cli_any_hit_counts_the_same_intersections(cli_case):
    """a ray is occluded iff it has a nearest hit."""
    c = cli_case
    r = _subproc.check([c.exe, c.obj, "-r", c.rays, "-k", "--any-hit"])
    assert f"{c.want} intersection(s)." in r.stdout


@pytest.mark.gpu
def test_cli_step_count_heat_map(cli_case):
    """The step-count picture of the viewer (main.cpp:100-107), written from the statistics entry point."""
    c = cli_case
    heat = os.path.join(c.dir, "steps.pgm")
    r = _subproc.check([c.exe, "soup:20000", "-sx", "128", "-sy", "64", "-s", heat])
    assert "Steps per ray: max " in r.stdout, r.stdout + r.stderr
    assert os.path.getsize(heat) == len("P5\n128 64\n255\n") + 128 * 64


@pytest.mark.gpu
def test_cli_save_grid_then_load_grid(cli_case):
    """The grid as a file: --save-grid, then --load-grid instead of a scene gives the same grid and the same intersections."""
    c = cli_case
    gfile = os.path.join(c.dir, "soup.grid")
    r = _subproc.check([c.exe, c.obj, "-r", c.rays, "-k", "--save-grid", gfile])
    assert f"{c.want} intersection(s)." in r.stdout and os.path.getsize(gfile) % 128 == 0
    r = _subproc.check([c.exe, "--load-grid", gfile, "-r", c.rays])
    assert "5000 triangle(s)" in r.stdout and "Grid loaded (" in r.stdout and f"{c.cells} cells, {c.refs} references)" in r.stdout
    assert f"{c.want} intersection(s)." in r.stdout


@pytest.mark.gpu
def test_cli_one_process_per_gpu_rccl_broadcast(cli_case):
    """One process per GPU, the grid broadcast from C++ with RCCL (here: one rank, all this box has)."""
    c = cli_case
    # (RCCL's first initialisation on a fresh box loads its kernels and probes the topology: tens of seconds on a slow host)
    r = _subproc.check([c.exe, c.obj, "-r", c.rays, "-k", "--gpus", "1", "-n", "2"], timeout=300)
    assert "1 rank(s), grid broadcast in " in r.stdout and f"{c.cells} cells, {c.refs} references)" in r.stdout
    assert f"{c.want} intersection(s)." in r.stdout and " Mrays/sec." in r.stdout


@pytest.mark.gpu
def test_plain_c_user_of_the_abi_on_gpu():
    """tests/cpp/c_abi_user.c (C99, the whole ABI incl. binning and options) driven through ctypes: hits == Python API's."""
    import ctypes as C
    import numpy as np
    import torch
    from hagrid_amd import api, lib, scene
    lib.load()                                                   # makes the HIP runtime + libhagrid_amd visible
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libcuser.so")
        subprocess.run(["gcc", "-std=c99", "-O1", "-fPIC", "-shared", "-I", INC, os.path.join(ROOT, "tests", "cpp", "c_abi_user.c"), "-o", so,
                        "-L", os.path.join(ROOT, "hagrid_amd"), "-lhagrid_amd", "-Wl,-rpath," + os.path.join(ROOT, "hagrid_amd"),
                        "-Wl,--allow-shlib-undefined"], check=True)
        U = C.CDLL(so)
        tris = scene.make_soup(20000)
        lo, hi = scene.tris_bbox(tris)
        rays = scene.make_rays_incoherent(lo, hi, 30000, 12)
        hits = np.zeros(rays.shape[0], dtype=api.HIT_DTYPE)
        rc = U.run(tris.ctypes.data_as(C.c_void_p), tris.shape[0], rays.ctypes.data_as(C.c_void_p), rays.shape[0], hits.ctypes.data_as(C.c_void_p))
        assert rc == 0
        mem = api.MemManager(keep=True)
        d_tris = mem.upload(tris); g = api.build_all(mem, d_tris, tris.shape[0])
        d_rays = mem.upload(rays); d_hits = _poison.alloc_out(mem, 16 * rays.shape[0])
        api.traverse_grid(g, d_tris, d_rays, d_hits, rays.shape[0])
        want = _poison.fetch(mem, d_hits, api.HIT_DTYPE, rays.shape[0])
        _poison.assert_all_written(want)
        assert (hits["id"] == want["id"]).all() and (hits["t"].view(np.uint32) == want["t"].view(np.uint32)).all()
        mem.close()
