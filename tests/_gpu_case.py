"""What the GPU test files of the queries share (test_closest_gpu, test_nearest_k_gpu, test_segments_gpu, test_overlap_gpu, test_overlap_tris_gpu,
test_crossings_gpu, test_crossing_lists_gpu, test_fill_lattice_gpu, test_distance_lattice_gpu, test_multi_hit_gpu, test_filtered_gpu): the case of a module
(a manager, the triangles, Cell and SmallCell grids built on the device); the sequences that every query runs around its own launches (a traversal image
present and ray binning on; the nearest-hit path before and after; a grid released for traversal; counters that are added to); the build of a shim program
of tests/cpp; the kernel budget; the ctypes conversions and the lattice table of the refusal tests.  The fixtures stay in the test files, and so does every
assertion about a query's own answers.  tests/_host.py is the counterpart for the host programs and the CPU oracle's grids."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np

import _host
from hagrid_amd import scene

EINVAL, ERANGE = -1, -4


# ---- the case ---------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def upload_case(tris, name=None):
    """a `keep` manager with the triangles uploaded: api, name, tris, mem, d_tris"""
    from hagrid_amd import api
    c = Case()
    c.api, c.name, c.tris = api, name, tris
    c.mem = api.MemManager(keep=True)
    c.d_tris = c.mem.upload(tris)
    return c


def open_case(name, tris):
    """upload_case and grids: {False: the Cell grid, True: the SmallCell grid}, built on the device, each what it claims to be; the caller closes c.mem"""
    c = upload_case(tris, name)
    c.grids = {False: c.api.build_all(c.mem, c.d_tris, tris.shape[0]), True: c.api.build_all(c.mem, c.d_tris, tris.shape[0], compress=True)}
    assert c.grids[True].small_cells and not c.grids[False].small_cells
    return c


# ---- the sequences around a query's own launches ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def image_present(c, grid, binning=False):
    """"traverse.image" = 2 and the grid's traversal image made, before the body and still after it; binning: ray binning on from the start (else the body
    switches it on where it wants it).  Binning is off afterwards, whatever the body did; "traverse.image" stays 2 and the image stays."""
    mem = c.mem
    mem.set_option("traverse.image", 2)
    c.api.setup_traversal(grid)
    assert mem.image_bytes(grid) > 0
    try:
        if binning:
            mem.set_ray_binning(1)
        yield
    finally:
        mem.set_ray_binning(0)
    assert mem.image_bytes(grid) > 0, "the query dropped the traversal image"


def drop_image(c, grid):
    """"traverse.image" = 0 and the grid's image gone; the option stays 0"""
    c.mem.set_option("traverse.image", 0)
    c.api.setup_traversal(grid)
    assert c.mem.image_bytes(grid) == 0


@contextlib.contextmanager
def nearest_hit_unmoved(c, grid, d_rays=0, num_rays=0):
    """a nearest-hit launch before the body and one after it (64 x 64 primary rays, or the caller's ray buffer): the hints kept for the ray buffer are
    unchanged by the body, the hits equal bit for bit, and some ray hits.  Yields an object with `before`, and `after` once the body is over."""
    api, mem = c.api, c.mem
    own = not d_rays
    if own:
        rays = scene.make_rays_primary(grid.bbox_min, grid.bbox_max, 64, 64)
        num_rays = rays.shape[0]
        d_rays = mem.upload(rays)
    d_hits = mem.alloc(16 * num_rays)

    def nearest():
        mem.one(d_hits, 16 * num_rays)
        api.traverse_grid(grid, c.d_tris, d_rays, d_hits, num_rays)
        mem.synchronize()
        return mem.download(d_hits, api.HIT_DTYPE, num_rays)

    run = types.SimpleNamespace(before=nearest(), after=None)
    state = mem.order_state(d_rays)
    yield run
    assert mem.order_state(d_rays) == state, "the hints of the nearest-hit path moved"
    run.after = nearest()
    mem.free(d_hits)
    if own:
        mem.free(d_rays)
    assert (run.before.view(np.uint32) == run.after.view(np.uint32)).all() and (run.before["id"] >= 0).any()


@contextlib.contextmanager
def released_grid(c, grid=None):
    """a second grid of the case's triangles (or the caller's), given up for traversal: "traverse.image" = 2, setup_traversal, release_for_traversal.  Yields
    the grid, or None where no image was made and nothing could be released; frees it afterwards."""
    api, mem = c.api, c.mem
    g2 = grid if grid is not None else api.build_all(mem, c.d_tris, c.tris.shape[0])
    try:
        mem.set_option("traverse.image", 2)
        api.setup_traversal(g2)
        released = mem.image_bytes(g2) > 0
        if released:
            api.release_for_traversal(g2)
        yield g2 if released else None
    finally:
        g2.free()


def assert_totals_added(launch, mem, tot):
    """the totals are ADDED: launch(d_tot) on counters that hold `tot`, the totals of the same launch, doubles them"""
    d_tot = mem.upload(tot)
    launch(d_tot)
    mem.synchronize()
    assert (mem.download(d_tot, np.int64, tot.size) == 2 * tot).all()
    mem.free(d_tot)


# ---- programs and tools -----------------------------------------------------------------------------------------------------------------------------------
def build_shim(name, directory):
    """tests/cpp/<name>_shim.cpp as a program in `directory`, linked against the product library and the HIP runtime torch ships"""
    import torch
    hip_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    exe = os.path.join(str(directory), name + "_shim")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", _host.INC, os.path.join(_host.ROOT, "tests", "cpp", name + "_shim.cpp"),
                    "-o", exe, "-L", os.path.join(_host.ROOT, "hagrid_amd"), "-lhagrid_amd", "-L", hip_lib, "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(_host.ROOT, "hagrid_amd"), "-Wl,-rpath," + hip_lib, "-Wl,--allow-shlib-undefined"], check=True)
    return exe


MAX_KERNELS = 120
KERNEL_COUNT = r"(\d+) kernels in"


def kernel_listing():
    """what tools/count_kernels.py -v prints for the product library"""
    return subprocess.run([sys.executable, os.path.join(_host.ROOT, "tools", "count_kernels.py"), "-v"], capture_output=True, text=True, check=True).stdout


def kernel_budget(listing, one_each=(), absent=()):
    """at most MAX_KERNELS kernels in the listing; every name of one_each occurs exactly once in it, no name of absent at all"""
    m = re.search(KERNEL_COUNT, listing)
    assert m and int(m.group(1)) <= MAX_KERNELS, listing[-300:]
    for name in one_each:
        assert listing.count(name) == 1, f"{name}: {listing.count(name)} times in the listing, not once"
    for name in absent:
        assert name not in listing, f"{name} is in the listing"


# ---- refusal tests ----------------------------------------------------------------------------------------------------------------------------------------
def pod(grid):
    return C.byref(grid.pod) if grid is not None else None


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v]) if v is not None else None


def i3(v):
    return (C.c_int * 3)(*[int(x) for x in v]) if v is not None else None


def vp(p):
    return C.c_void_p(p) if p is not None else None


_O, _S, _N = (0, 0, 0), (1, 1, 1), (2, 2, 2)
# (origin, size, n), each refused with HAGRID_EINVAL by every entry point that takes a lattice: a count that is not positive, more than 2^31 - 1 voxels (in the
# plane, in all), a size that is not positive and finite, an origin that is not finite, a null array
LATTICES_REFUSED = (
    [(_O, _S, n) for n in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1 << 16, 1 << 16, 1), (1 << 11, 1 << 10, 1 << 10), (1 << 30, 1, 4))]
    + [(_O, s, _N) for s in ((0, 1, 1), (1, -1, 1), (1, 1, float("nan")), (float("inf"), 1, 1), (0.1, 0.0, 0.1), (0.1, float("inf"), 0.1), (float("nan"), 1, 1))]
    + [(o, _S, _N) for o in ((float("nan"), 0, 0), (0, float("-inf"), 0), (0, float("inf"), 0))]
    + [(None, _S, _N), (_O, None, _N), (_O, _S, None)])


def assert_lattice_refused(call):
    """call(origin, size, n) -> the entry point's status, its other arguments valid: every lattice of LATTICES_REFUSED is refused with HAGRID_EINVAL"""
    for origin, size, n in LATTICES_REFUSED:
        status = call(origin, size, n)
        assert status == EINVAL, f"origin {origin}, size {size}, n {n}: status {status}"
