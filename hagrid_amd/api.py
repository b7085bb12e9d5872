"""Host-side mirror of the reference's operator interface for the hot path, over the C ABI.

Same names, argument meaning and error behaviour as the reference's C++ API so that tests read like
the reference's own call sequence (main.cpp:471-506, :535, :410-425):

    mem  = MemManager(keep=True)                        # mem_manager.h:34-119
    tris = mem.upload(host_tris)                        # mem.alloc<Tri> + copy<HST_TO_DEV>
    grid = Grid()
    build_grid(mem, tris, n, grid, 0.12, 2.4)           # build.h:17
    merge_grid(mem, grid, 0.995)                        # build.h:20
    flatten_grid(mem, grid)                             # build.h:25
    expand_grid(mem, grid, tris, 3)                     # build.h:28
    compress_grid(mem, grid)                            # build.h:31 (bool)
    setup_traversal(grid)                               # traverse.h:11
    traverse_grid(grid, tris, rays, hits, num_rays)     # traverse.h:14
    ms = profile(lambda: traverse_grid(...))            # common.h:15

Device buffers are plain integer addresses (what the C ABI takes).  Errors raise HagridError carrying the
"file(line): message" text -- the reference prints that text and abort()s (common.h:103-108).
There is no CPU path here: without the compiled library and a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import lib as _lib
from .lib import Camera, GridPOD, HagridError, TraversalStats
from .scene import BOX_QUERY_DTYPE, OBB_DTYPE, CELL_DTYPE, CLOSEST_DTYPE, HIT_DTYPE, NEAREST_ENTRY_DTYPE, POINT_QUERY_DTYPE, SEGMENT_DTYPE, SEGMENT_RECORD_DTYPE, SMALL_CELL_DTYPE

_current = None  # the most recently created MemManager (profile / setup_traversal take no manager)


def _check(mem: "MemManager", rc: int, what: str) -> int:
    if rc < 0:
        msg = _lib.load().hagrid_last_error(mem._ctx)
        raise HagridError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc


class MemManager:
    """Buffer pool on one GPU (reference: MemManager, mem_manager.h:34-119).  `keep` retains freed
    buffers between builds (README.md:52-54 recommends it for build benchmarks)."""

    def __init__(self, keep: bool = False, device: int | None = None):
        global _current
        L = _lib.load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        h = C.c_void_p()
        rc = L.hagrid_ctx_create(C.byref(h), int(device), 1 if keep else 0)
        if rc != 0 or not h:
            raise HagridError(f"hagrid_ctx_create(device={device}) failed ({rc}): no usable gfx950 device")
        self._L = L
        self._ctx = h
        self.device = int(device)
        _current = self

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.hagrid_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_stream(self, stream: int | None):
        """Enqueue all further work on a hipStream_t given as an integer (e.g. torch's cuda_stream)."""
        _check(self, self._L.hagrid_ctx_set_stream(self._ctx, C.c_void_p(stream or 0)), "set_stream")
        self._stream = int(stream or 0)

    def torch_stream(self):
        """the manager's stream as a torch stream: torch work queued under `with torch.cuda.stream(mem.torch_stream())` is ordered with the manager's launches"""
        import torch
        s = getattr(self, "_stream", 0)
        return torch.cuda.ExternalStream(s, device=self.device) if s else torch.cuda.default_stream(self.device)

    def synchronize(self):
        """Waits for everything queued on this manager's stream (hagrid_ctx_synchronize)."""
        _check(self, self._L.hagrid_ctx_synchronize(self._ctx), "synchronize")

    def set_ray_binning(self, mode: int):
        """Extension: 1 = bin each ray batch by grid-entry position before traversal (for incoherent batches);
        2 = automatic: the device bins a batch only if it is neither image-ordered nor coherent (no host round trip)."""
        _check(self, self._L.hagrid_set_ray_binning(self._ctx, int(mode)), "set_ray_binning")

    PRODUCT_OPTIONS = ("expand.subset_only", "traverse.id_is_steps", "traverse.image", "traverse.image_max_mb", "traverse.image_width", "traverse.tile_order")

    def set_option(self, key: str, value: int):
        """The product's options (include/hagrid_amd.h: hagrid_set_option); any other key is a code-path selector of the test library
        (csrc/kat/hagrid_amd_kat.h: hagrid_kat_set_option -- tests and dev tools).  Hits never depend on either."""
        if key in self.PRODUCT_OPTIONS:
            _check(self, self._L.hagrid_set_option(self._ctx, key.encode(), int(value)), f"set_option({key})")
        else:
            _check(self, self._K.hagrid_kat_set_option(self._ctx, key.encode(), int(value)), f"kat_set_option({key})")

    def scan_epoch(self) -> int:
        """tests: the epoch of the look-back scans' status words (csrc/kat/hagrid_amd_kat.h: hagrid_kat_scan_epoch; "scan.epoch" sets it)"""
        e = C.c_int32(-1)
        _check(self, self._K.hagrid_kat_scan_epoch(self._ctx, C.byref(e)), "scan_epoch")
        return int(e.value)

    MEM_STATE_KEYS = ("requests", "mallocs", "slots_in_use", "tracked", "bytes_in_use", "bytes_cached")

    def mem_state(self) -> dict:
        """tests: the allocation layer's books (csrc/kat/hagrid_amd_kat.h: hagrid_kat_mem_state; "mem.fail_request" / "mem.fail_malloc" inject failures)"""
        out = (C.c_int64 * 6)()
        _check(self, self._K.hagrid_kat_mem_state(self._ctx, out), "mem_state")
        return dict(zip(self.MEM_STATE_KEYS, (int(v) for v in out)))

    def mem_retry(self) -> dict:
        """tests: the retry branch of hagrid_mem_alloc (csrc/kat/hagrid_amd_kat.h: hagrid_kat_mem_retry)"""
        out = (C.c_int64 * 4)()
        _check(self, self._K.hagrid_kat_mem_retry(self._ctx, out), "mem_retry")
        return dict(zip(("retries", "bytes_given_back", "cached_behind", "usage_minus_in_use_behind"), (int(v) for v in out)))

    def mem_pending(self) -> tuple:
        """tests: ("mem.fail_request", "mem.fail_malloc", "mem.fail_scan") as they stand -- 0 once they have fired"""
        a = C.c_int32(-1); b = C.c_int32(-1); c = C.c_int32(-1)
        _check(self, self._K.hagrid_kat_mem_pending(self._ctx, C.byref(a), C.byref(b), C.byref(c)), "mem_pending")
        return int(a.value), int(b.value), int(c.value)

    def forget_hints(self):
        """dev tools: the context forgets every ray buffer it has traversed (csrc/kat/hagrid_amd_kat.h: hagrid_kat_forget_hints)"""
        _check(self, self._K.hagrid_kat_forget_hints(self._ctx), "forget_hints")

    def order_state(self, d_rays) -> dict:
        """dev tools / tests: what the context remembers about a ray buffer's tile order (csrc/kat/hagrid_amd_kat.h: hagrid_kat_order_state)"""
        out = (C.c_int32 * 12)(); ms = (C.c_float * 4)()
        _check(self, self._K.hagrid_kat_order_state(self._ctx, C.c_void_p(d_rays), out, ms), "order_state")
        keys = ("slot", "valid", "cooling", "head_tiles", "head_dropped", "n_base", "n_head", "share_choice", "share_samples", "n_all", "head_suggested", "share_launches")
        d = dict(zip(keys, list(out))); d["ms_base"] = round(ms[0], 4); d["ms_head"] = round(ms[1], 4); d["ms_all"] = round(ms[2], 4); d["ms_share_best"] = round(ms[3], 4)
        d["order_loses"] = d["share_samples"] >= 10000; d["share_samples"] %= 10000; d["cooldown"] = d["n_all"] // 100; d["learned_all"] = (d["n_all"] // 10) % 10 == 1; d["n_all"] %= 10
        return d

    def device_info(self) -> dict:
        name = C.create_string_buffer(128); cus = C.c_int(); mem = C.c_int64()
        _check(self, self._L.hagrid_device_info(self._ctx, name, 128, C.byref(cus), C.byref(mem)), "device_info")
        return {"arch": name.value.decode(), "compute_units": cus.value, "total_mem": mem.value}

    # -- alloc / free / copy / zero / one ------------------------------------------------------------
    def alloc(self, nbytes: int) -> int:
        p = self._L.hagrid_mem_alloc(self._ctx, int(nbytes))
        if not p:
            raise HagridError("alloc failed: " + self._L.hagrid_last_error(self._ctx).decode())
        return int(p)

    def free(self, ptr: int | None):
        if ptr:
            _check(self, self._L.hagrid_mem_free(self._ctx, C.c_void_p(ptr)), "free")

    def copy_h2d(self, dst: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        _check(self, self._L.hagrid_mem_copy_h2d(self._ctx, C.c_void_p(dst), src.ctypes.data_as(C.c_void_p), src.nbytes), "copy h2d")

    def copy_d2h(self, dst: np.ndarray, src: int):
        assert dst.flags["C_CONTIGUOUS"]
        _check(self, self._L.hagrid_mem_copy_d2h(self._ctx, dst.ctypes.data_as(C.c_void_p), C.c_void_p(src), dst.nbytes), "copy d2h")

    def copy_d2d(self, dst: int, src: int, nbytes: int):
        _check(self, self._L.hagrid_mem_copy_d2d(self._ctx, C.c_void_p(dst), C.c_void_p(src), int(nbytes)), "copy d2d")

    def zero(self, ptr: int, nbytes: int):
        _check(self, self._L.hagrid_mem_zero(self._ctx, C.c_void_p(ptr), int(nbytes)), "zero")

    def one(self, ptr: int, nbytes: int):
        _check(self, self._L.hagrid_mem_one(self._ctx, C.c_void_p(ptr), int(nbytes)), "one")

    def usage(self) -> int:
        return int(self._L.hagrid_mem_usage(self._ctx))

    def max_usage(self) -> int:
        return int(self._L.hagrid_mem_max_usage(self._ctx))

    def debug_slots(self):
        self._L.hagrid_mem_debug_slots(self._ctx)

    def bandwidth_probe(self, nbytes: int = 1 << 30, iters: int = 5) -> dict:
        """Measured device copy / triad bandwidth in GB/s (SURVEY.md 8(d) BW_peak, 'measured in the same run')."""
        c = C.c_float(); t = C.c_float()
        _check(self, self._L.hagrid_bandwidth_probe(self._ctx, int(nbytes), int(iters), C.byref(c), C.byref(t)), "bandwidth_probe")
        return {"copy_GBps": float(c.value), "triad_GBps": float(t.value)}

    def image_format(self, grid: "Grid") -> dict:
        """Layout of the traversal image held for `grid`: flat / uniform (table-free) / general (a slim record per voxel-map entry) / slim id bits /
        bytes per record ({} without an image)."""
        f = (C.c_int32 * 4)()
        if self._L.hagrid_traversal_image_info(self._ctx, C.byref(grid.pod), f, None) != 0:
            return {}
        return {"flat": bool(f[0]), "uniform": bool(f[1] & 1), "general": f[0] == 2, "slim_id_bits": int(f[2]), "record_bytes": int(f[3]), "two_layouts": bool(f[1] & 2)}

    def image_record_bytes(self, grid: "Grid") -> int:
        """16 when the traversal image of `grid` holds slim records, else 32."""
        return self.image_format(grid).get("record_bytes", 32)

    def image_bytes(self, grid: "Grid") -> int:
        """Size of the traversal image this manager holds for `grid` (0 when it holds none)."""
        b = C.c_int64(0)
        rc = self._L.hagrid_traversal_image_info(self._ctx, C.byref(grid.pod), None, C.byref(b))
        return int(b.value) if rc == 0 else 0

    @property
    def _K(self):
        """libhagrid_amd_kat.so: known-answer hooks and timed diagnostic kernels (tests and dev tools only)."""
        return _lib.load_kat()

    def build_counts(self) -> dict:
        """Sizes the construction passes of this manager went through since its last build_grid."""
        bc = _lib.BuildCounts()
        _check(self, self._L.hagrid_get_build_counts(self._ctx, C.byref(bc)), "get_build_counts")
        return bc.as_dict()

    # -- conveniences ----------------------------------------------------------------------------------
    def upload(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = self.alloc(max(arr.nbytes, 4))
        if arr.nbytes:
            self.copy_h2d(p, arr)
        return p

    def download(self, ptr: int, dtype, count: int) -> np.ndarray:
        out = np.empty(int(count), dtype=dtype)
        if out.nbytes:
            self.copy_d2h(out, ptr)
        return out


class Grid:
    """The reference's `struct Grid` (grid.h:48-62); device pointers are integers."""

    def __init__(self):
        self.pod = GridPOD()
        self.mem: MemManager | None = None

    entries = property(lambda s: s.pod.entries or 0)
    ref_ids = property(lambda s: s.pod.ref_ids or 0)
    cells = property(lambda s: s.pod.cells or 0)
    small_cells = property(lambda s: s.pod.small_cells or 0)
    dims = property(lambda s: tuple(s.pod.dims))
    shift = property(lambda s: int(s.pod.shift))
    num_cells = property(lambda s: int(s.pod.num_cells))
    num_entries = property(lambda s: int(s.pod.num_entries))
    num_refs = property(lambda s: int(s.pod.num_refs))
    offsets = property(lambda s: [int(s.pod.offsets[i]) for i in range(s.pod.num_offsets)])
    bbox_min = property(lambda s: np.array(list(s.pod.bbox_min), dtype=np.float32))
    bbox_max = property(lambda s: np.array(list(s.pod.bbox_max), dtype=np.float32))

    def summary(self) -> dict:
        return {"dims": self.dims, "shift": self.shift, "num_cells": self.num_cells, "num_refs": self.num_refs,
                "num_entries": self.num_entries, "offsets": self.offsets, "compressed": bool(self.small_cells)}

    def free(self, mem: MemManager | None = None):
        """mem.free(grid.entries / cells / ref_ids [/ small_cells]) as main.cpp:496-498 does."""
        mem = mem or self.mem
        for f in ("entries", "cells", "ref_ids", "small_cells"):
            p = getattr(self.pod, f)
            if p:
                mem.free(p)
                setattr(self.pod, f, None)

    def download(self, mem: MemManager | None = None) -> dict:
        mem = mem or self.mem
        d = {"entries": mem.download(self.entries, np.uint32, self.num_entries),
             "ref_ids": mem.download(self.ref_ids, np.int32, self.num_refs),
             "cells": mem.download(self.cells, CELL_DTYPE, self.num_cells) if self.cells else None,
             "small_cells": mem.download(self.small_cells, SMALL_CELL_DTYPE, self.num_cells) if self.small_cells else None}
        d.update(bbox_min=self.bbox_min, bbox_max=self.bbox_max, dims=self.dims, shift=self.shift, offsets=self.offsets)
        return d

    @staticmethod
    def load(mem: MemManager, path: str) -> tuple["Grid", int, int]:
        """A grid file written by hagrid_grid_save (hagrid_cli --save-grid): (grid, device pointer of its triangles, their number)."""
        g = Grid(); g.mem = mem
        tris = C.c_void_p(); n = C.c_int32()
        _check(mem, mem._L.hagrid_grid_load(mem._ctx, path.encode(), C.byref(g.pod), C.byref(tris), C.byref(n)), "grid_load")
        return g, tris.value, n.value

    @staticmethod
    def upload(mem: MemManager, entries, ref_ids, cells, small_cells, bbox_min, bbox_max, dims, shift, offsets) -> "Grid":
        """Assemble a device grid from host arrays (fixtures, the broadcast blob of dist.py)."""
        g = Grid(); g.mem = mem
        g.pod.entries = mem.upload(np.ascontiguousarray(entries, dtype=np.uint32))
        g.pod.ref_ids = mem.upload(np.ascontiguousarray(ref_ids, dtype=np.int32))
        n_cells = 0
        if cells is not None:
            g.pod.cells = mem.upload(cells); n_cells = len(cells)
        if small_cells is not None:
            g.pod.small_cells = mem.upload(small_cells); n_cells = len(small_cells)
        for i in range(3):
            g.pod.bbox_min[i] = float(bbox_min[i]); g.pod.bbox_max[i] = float(bbox_max[i]); g.pod.dims[i] = int(dims[i])
        g.pod.num_cells = n_cells; g.pod.num_entries = len(entries); g.pod.num_refs = len(ref_ids)
        g.pod.shift = int(shift); g.pod.num_offsets = len(offsets)
        for i, o in enumerate(offsets):
            g.pod.offsets[i] = int(o)
        return g


# ---- build.h -----------------------------------------------------------------------------------------

def build_grid(mem: MemManager, tris: int, num_tris: int, grid: Grid, top_density: float, snd_density: float):
    grid.mem = mem
    _check(mem, mem._L.hagrid_build_grid(mem._ctx, C.c_void_p(tris), int(num_tris), C.byref(grid.pod), top_density, snd_density), "build_grid")


def merge_grid(mem: MemManager, grid: Grid, alpha: float):
    _check(mem, mem._L.hagrid_merge_grid(mem._ctx, C.byref(grid.pod), alpha), "merge_grid")


def flatten_grid(mem: MemManager, grid: Grid):
    _check(mem, mem._L.hagrid_flatten_grid(mem._ctx, C.byref(grid.pod)), "flatten_grid")


def expand_grid(mem: MemManager, grid: Grid, tris: int, iters: int):
    _check(mem, mem._L.hagrid_expand_grid(mem._ctx, C.byref(grid.pod), C.c_void_p(tris), int(iters)), "expand_grid")


def compress_grid(mem: MemManager, grid: Grid) -> bool:
    return _check(mem, mem._L.hagrid_compress_grid(mem._ctx, C.byref(grid.pod)), "compress_grid") == 1


def build_all(mem: MemManager, tris: int, num_tris: int, top_density=0.12, snd_density=2.4, alpha=0.995,
              exp_iters=3, compress=False, grid: Grid | None = None) -> Grid:
    """The construction sequence of main.cpp:500-506."""
    grid = grid or Grid()
    build_grid(mem, tris, num_tris, grid, top_density, snd_density)
    merge_grid(mem, grid, alpha)
    flatten_grid(mem, grid)
    expand_grid(mem, grid, tris, exp_iters)
    if compress:
        compress_grid(mem, grid)
    return grid


# ---- traverse.h ---------------------------------------------------------------------------------------

def setup_traversal(grid: Grid):
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_setup_traversal(mem._ctx, C.byref(grid.pod)), "setup_traversal")


def release_for_traversal(grid: Grid):
    """Extension: frees grid.entries and grid.cells | small_cells once setup_traversal has built a self-contained traversal image;
    traverse_grid keeps working (hagrid_grid_release_for_traversal)."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_grid_release_for_traversal(mem._ctx, C.byref(grid.pod)), "release_for_traversal")


def share_traversal(dst: MemManager, grid: Grid) -> Grid:
    """Extension (hagrid_share_traversal): a descriptor of `grid` for the context `dst` (another stream on the same device) that
    traverses with the traversal image of grid.mem instead of a copy of its own -- independent batches in flight over one image.
    The arrays and the image stay the property of grid.mem."""
    src = grid.mem or _current
    _check(dst, dst._L.hagrid_share_traversal(dst._ctx, src._ctx), "share_traversal")
    g = Grid(); g.mem = dst
    C.memmove(C.byref(g.pod), C.byref(grid.pod), C.sizeof(grid.pod))
    return g


ANY_HIT, UVS = 1, 2      # hagrid_traverse_grid_ex flags


def traverse_grid(grid: Grid, tris: int, rays: int, hits: int, num_rays: int, flags: int = 0):
    """traverse_grid (traverse.h:14); flags: ANY_HIT (shadow rays: stop at the first accepted intersection) | UVS
    (barycentrics stored with the hit, the reference's COMPUTE_UVS build)."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_traverse_grid_ex(mem._ctx, C.byref(grid.pod), C.c_void_p(tris), C.c_void_p(rays), C.c_void_p(hits), int(num_rays), int(flags)), "traverse_grid")


MAX_HITS = 8             # HAGRID_MAX_HITS


def traverse_grid_multi(grid: Grid, tris: int, rays: int, hits: int, num_rays: int, k: int, flags: int = 0):
    """Extension (hagrid_traverse_grid_multi): the k nearest intersections of every ray, sorted by (t, id), into hits[i * k .. i * k + k - 1]
    (num_rays * k Hit records); unused slots are misses (id -1, t = tmax).  1 <= k <= MAX_HITS; flags: 0 | UVS.  Walks the construction
    format: not for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_traverse_grid_multi(mem._ctx, C.byref(grid.pod), C.c_void_p(tris), C.c_void_p(rays), C.c_void_p(hits), int(num_rays), int(k), int(flags)), "traverse_grid_multi")


RAY_MASK_ALL = 0xFFFFFFFF  # HAGRID_RAY_MASK_ALL


def traverse_grid_filtered(grid: Grid, tris: int, rays: int, hits: int, num_rays: int, k: int, filters: int = 0, tri_masks: int = 0, flags: int = 0):
    """Extension (hagrid_traverse_grid_filtered): traverse_grid_multi over the triangles that TAKE PART for each ray -- triangle j for ray i exactly
    when (mask_i & tri_masks[j]) != 0 and j != skip_i.  filters: 0 (every ray sees everything) or the address of num_rays records of 8 bytes, int32 pairs
    (mask, skip) -- what skip_filters makes; skip < 0 skips nothing.  tri_masks: 0 (all ones) or one 32-bit mask per triangle -- what
    MeshScene.instance_masks makes.  hits: num_rays * k Hit records, the layout and order of traverse_grid_multi.  flags: 0 | UVS | ANY_HIT; ANY_HIT
    needs k = 1 and reports SOME candidate, not a promised one (occlusion rays: skip = the triangle the ray starts on, tmin = 0).  Asynchronous on the manager's stream."""
    mem = grid.mem
    _check(mem, mem._L.hagrid_traverse_grid_filtered(mem._ctx, C.byref(grid.pod), C.c_void_p(tris), C.c_void_p(rays), C.c_void_p(filters or 0), C.c_void_p(tri_masks or 0),
                                                     C.c_void_p(hits), int(num_rays), int(k), int(flags)), "traverse_grid_filtered")


def skip_filters(hits, mask: int = RAY_MASK_ALL, mem: MemManager | None = None):
    """The filter records that make every ray skip the triangle of a hit: hits is a torch tensor of n Hit records as 4 x int32 (shape (n, 4), or anything
    that views as it: the output of traverse_grid on the device); returns the (n, 2) int32 tensor (mask, skip = hits.id) for traverse_grid_filtered -- a
    miss (id -1) skips nothing.  Torch operations on the manager's stream, no kernel of this library."""
    import torch
    mem = mem or _current
    m = int(mask) & 0xFFFFFFFF
    with torch.cuda.stream(mem.torch_stream()):
        h = hits.view(torch.int32).reshape(-1, 4)
        out = torch.empty((h.shape[0], 2), dtype=torch.int32, device=h.device)
        out[:, 0] = m - (1 << 32) if m >= (1 << 31) else m
        out[:, 1] = h[:, 0]
    return out


def closest_points(grid: Grid, tris: int, points: int, results: int, n: int, counters: int = 0):
    """Extension (hagrid_closest_points): for each of n points (16 bytes: x, y, z, r -- POINT_QUERY_DTYPE) the nearest triangle within r: 32 bytes
    per query into `results` (CLOSEST_DTYPE: q, d2, id, feature, side); nothing within r: id -1, d2 = r * r, q = p.  counters: 0, or a device int64[4]
    the batch totals are added to (queries, cells visited, triangles tested, sub-blocks pruned).  All arguments are device addresses (a torch tensor
    passes as t.data_ptr()); asynchronous on the manager's stream.  scene.closest_points states the results in numpy, bit for bit.  Walks the
    construction format: not for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_closest_points(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(points or 0), C.c_void_p(results or 0), int(n),
                                             C.c_void_p(counters or 0), 0), "closest_points")


MAX_NEAREST = 8          # HAGRID_MAX_NEAREST


def nearest_tris(grid: Grid, tris: int, points: int, n: int, k: int, entries: int = 0, records: int = 0, cursors: int = 0, query_labels: int = 0,
                 tri_labels: int = 0, counters: int = 0):
    """Extension (hagrid_nearest_tris): NEIGHBOUR queries -- for each of n points (POINT_QUERY_DTYPE: x, y, z, r) the k nearest triangles within r, nearest
    first: entries[i * k .. i * k + k - 1] (NEAREST_ENTRY_DTYPE: d2, id; unused slots d2 = r * r, id -1) and / or records (k CLOSEST_DTYPE records per
    query); one of the two may be 0.  1 <= k <= MAX_NEAREST.  cursors: 0, or one entry per query -- only what sorts after it in (d2, id) is listed; the
    cursor of the next page is the last slot of a FULL list, a list that is not full is the last page.  query_labels (int32[n]) and tri_labels (int32[3 per
    scene triangle]): both or neither; a triangle that carries the query's label (>= 0) is left out (MeshScene.vertex_labels with label = vertex index: a
    vertex does not see its own triangles).  counters: 0, or a device int64[5] the batch totals are added to (queries, cells visited, triangles tested,
    sub-blocks pruned, lists that came back full).  All arguments are device addresses (a torch tensor passes as t.data_ptr()); asynchronous on the
    manager's stream.  scene.nearest_tris states the results in numpy, bit for bit.  Walks the construction format: not for a grid given up with
    release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_nearest_tris(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(points or 0), int(n), int(k), C.c_void_p(cursors or 0),
                                           C.c_void_p(query_labels or 0), C.c_void_p(tri_labels or 0), C.c_void_p(entries or 0), C.c_void_p(records or 0),
                                           C.c_void_p(counters or 0), 0), "nearest_tris")


def _paged_csr(launch, width: int, grid: Grid, tris, queries, k: int, query_labels, tri_labels, max_pages) -> dict:
    """tris_within and tris_near_segments: launch (nearest_tris or segment_tris) paged on torch tensors into CSR; width: float32 words per query"""
    import torch
    ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
    k = int(k)
    pts = queries.reshape(-1, width)
    n = int(pts.shape[0])
    dev = pts.device
    active = torch.arange(n, dtype=torch.int64, device=dev)                 # the queries of this page
    cur_pts, cur_lab, cursors = pts, query_labels, None
    page_q, page_e = [], []
    counters = torch.zeros(5, dtype=torch.int64, device=dev)
    pages, complete = 0, True
    while active.numel():
        if max_pages is not None and pages >= int(max_pages):
            complete = False
            break
        pages += 1
        m = int(active.numel())
        entries = torch.empty((m, k, 2), dtype=torch.int32, device=dev)
        counters.zero_()
        launch(grid, ptr(tris), cur_pts.data_ptr(), m, k, entries=entries.data_ptr(), cursors=ptr(cursors),
               query_labels=ptr(cur_lab) if query_labels is not None else 0, tri_labels=ptr(tri_labels) if query_labels is not None else 0,
               counters=counters.data_ptr())
        page_q.append(active); page_e.append(entries)
        if int(counters[4].item()) == 0:
            break
        full = entries[:, k - 1, 1] >= 0
        active = active[full]
        cur_pts = cur_pts[full].contiguous()
        cursors = entries[full][:, k - 1, :].contiguous()
        if query_labels is not None:
            cur_lab = cur_lab[full].contiguous()
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if not page_q:
        return {"offsets": offsets, "ids": torch.zeros(0, dtype=torch.int32, device=dev), "d2": torch.zeros(0, dtype=torch.float32, device=dev), "pages": 0,
                "complete": complete}
    # the entries of all pages, by query and -- pages being in list order -- by page inside a query: a stable sort by query
    q = torch.cat([a[:, None].expand(-1, k).reshape(-1) for a in page_q])
    e = torch.cat([x.reshape(-1, 2) for x in page_e])
    used = e[:, 1] >= 0
    q, e = q[used], e[used]
    order = torch.sort(q, stable=True)[1]
    e = e[order]
    torch.cumsum(torch.bincount(q, minlength=n), 0, out=offsets[1:])
    return {"offsets": offsets, "ids": e[:, 1].contiguous(), "d2": e[:, 0].contiguous().view(torch.float32), "pages": pages, "complete": complete}


def tris_within(grid: Grid, tris, points, k: int = MAX_NEAREST, query_labels=None, tri_labels=None, max_pages=None) -> dict:
    """ALL the triangles within r of every point, nearest first, in CSR form: nearest_tris paged on torch tensors.  Page by page the queries whose last list
    came back full are asked again behind their last entry; ONE scalar per page goes to the host (the fifth counter: how many lists were full).  tris,
    points ((n, 4) float32: x, y, z, r), query_labels ((n,) int32) and tri_labels ((N, 3) int32): torch tensors on the device (tris and tri_labels may be
    device addresses).  The manager must run on torch's current stream (mem.use_stream(torch.cuda.current_stream().cuda_stream)).  Returns "offsets" int64
    (n + 1,), "ids" int32 and "d2" float32 (total,): the triangles of point i are offsets[i] .. offsets[i + 1], sorted by (d2, id) -- what scene.tris_within
    states -- and "pages", how many launches it took, and "complete": False only when max_pages (None: no bound) ended the paging before every list had
    ended; the lists are then prefixes.  Meant for radii that hold tens of triangles: every page walks the ball of the pages before it again, so a list of L
    triangles costs L / k launches over O(L) triangles each, and r = inf lists the whole scene for every point, k at a time.  ball_lists gives the same lists
    in one pass."""
    return _paged_csr(nearest_tris, 4, grid, tris, points, k, query_labels, tri_labels, max_pages)


def ball_refs(grid: Grid, tris: int, points: int, n: int, counts: int = 0, offsets: int = 0, entries: int = 0, capacity: int = 0, query_labels: int = 0,
              tri_labels: int = 0, counters: int = 0):
    """Extension (hagrid_ball_refs): stage 1 of the BALL LISTS -- the walk of nearest_tris with a bound that stays r * r, so that it sees every candidate.  A
    REFERENCE is one accepted offer; a triangle arrives once per visit of a cell that lists it, so references hold duplicates.  Count mode (offsets = 0,
    entries = 0, capacity = 0): counts[i] (int32[n]) = R_i, the references of query i.  Fill mode: offsets int64[n + 1] -- query i owns the slots
    [offsets[i], offsets[i + 1]) of `entries` (capacity slots of NEAREST_ENTRY_DTYPE) and writes its first min(R_i, room) references in walk order, then the
    empty entry (+inf, -1); the room rule is list_crossings'.  counters: 0, or a device int64[6] added to (queries, cells visited, triangles tested,
    sub-blocks pruned, references written, queries that did not fit).  Device addresses; asynchronous on the manager's stream.  Walks the construction
    format: not for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_ball_refs(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(points or 0), int(n), C.c_void_p(query_labels or 0),
                                        C.c_void_p(tri_labels or 0), C.c_void_p(offsets or 0), C.c_void_p(counts or 0), C.c_void_p(entries or 0), int(capacity),
                                        C.c_void_p(counters or 0), 0), "ball_refs")


def unique_lists(num_lists: int, offsets: int, entries: int, capacity: int, counts: int, counters: int = 0, mem=None):
    """Extension (hagrid_unique_lists): stage 2 -- every segment [offsets[i], offsets[i + 1]) of `entries` in place: entries with id < 0 or a NaN d2 dropped, the
    rest sorted by (d2, id), equal ids reduced to one (equal ids must carry equal d2 bits), the survivors at the front, the empty entry behind them;
    counts[i] (int32) = how many survive.  Needs no grid.  counters: 0, or a device int64[4] added to (lists, slots, survivors, lists sorted in global
    memory).  scene.unique_lists states it in numpy.  mem: the manager whose stream it runs on (None: the most recent one)."""
    mem = mem or _current
    _check(mem, mem._L.hagrid_unique_lists(mem._ctx, int(num_lists), C.c_void_p(offsets or 0), C.c_void_p(entries or 0), int(capacity), C.c_void_p(counts or 0),
                                           C.c_void_p(counters or 0), 0), "unique_lists")


def compact_lists(num_lists: int, offsets: int, entries: int, capacity: int, counts: int, out_offsets: int, out_entries: int, out_capacity: int, counters: int = 0,
                  mem=None):
    """Extension (hagrid_compact_lists): stage 3 -- the first min(counts[i], room of the source, room of the destination) entries of segment i go to
    [out_offsets[i], out_offsets[i + 1]) of out_entries, the rest of that room gets the empty entry.  counters: 0, or a device int64[4] added to (lists,
    entries copied, lists cut short, 0).  scene.compact_lists states it in numpy."""
    mem = mem or _current
    _check(mem, mem._L.hagrid_compact_lists(mem._ctx, int(num_lists), C.c_void_p(offsets or 0), C.c_void_p(entries or 0), int(capacity), C.c_void_p(counts or 0),
                                            C.c_void_p(out_offsets or 0), C.c_void_p(out_entries or 0), int(out_capacity), C.c_void_p(counters or 0), 0), "compact_lists")


def ball_lists(grid: Grid, tris, points, query_labels=None, tri_labels=None) -> dict:
    """ALL the triangles within r of every point, nearest first, in CSR form, WITHOUT paging: ball_refs (count), torch.cumsum, ball_refs (fill), unique_lists,
    torch.cumsum, compact_lists on torch tensors; TWO scalars go to the host (the totals that size the scratch and the output).  Arguments as tris_within;
    the manager must run on torch's current stream (mem.use_stream(torch.cuda.current_stream().cuda_stream)).  Returns "offsets" int64 (n + 1,), "ids" int32
    and "d2" float32 (total,) exactly as tris_within does -- what scene.tris_within states -- and "refs", the total of R_i: the scratch (8 bytes each) a
    caller of the staged entry points needs.  Linear in the ball's content where tris_within is quadratic; r = inf lists the whole scene for every point."""
    import torch
    ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
    mem = grid.mem or _current
    pts = points.reshape(-1, 4)
    n = int(pts.shape[0])
    dev = pts.device
    ql = ptr(query_labels) if query_labels is not None else 0
    tl = ptr(tri_labels) if query_labels is not None else 0
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    ball_refs(grid, ptr(tris), pts.data_ptr(), n, counts=counts.data_ptr(), query_labels=ql, tri_labels=tl)
    ref_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum(counts, 0, dtype=torch.int64, out=ref_offsets[1:])
    refs = int(ref_offsets[-1].item())
    scratch = torch.empty((refs, 2), dtype=torch.int32, device=dev)
    ball_refs(grid, ptr(tris), pts.data_ptr(), n, offsets=ref_offsets.data_ptr(), entries=scratch.data_ptr() if refs else 0, capacity=refs, query_labels=ql, tri_labels=tl)
    unique_lists(n, ref_offsets.data_ptr(), scratch.data_ptr() if refs else 0, refs, counts.data_ptr(), mem=mem)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    total = int(offsets[-1].item())
    out = torch.empty((total, 2), dtype=torch.int32, device=dev)
    compact_lists(n, ref_offsets.data_ptr(), scratch.data_ptr() if refs else 0, refs, counts.data_ptr(), offsets.data_ptr(), out.data_ptr() if total else 0, total, mem=mem)
    return {"offsets": offsets, "ids": out[:, 1].contiguous(), "d2": out[:, 0].contiguous().view(torch.float32), "refs": refs}


def segment_tris(grid: Grid, tris: int, segments: int, n: int, k: int, entries: int = 0, records: int = 0, cursors: int = 0, query_labels: int = 0,
                 tri_labels: int = 0, counters: int = 0):
    """Extension (hagrid_segment_tris): CAPSULE queries -- for each of n segments (SEGMENT_DTYPE: a, r, b, 0) the k triangles nearest to the SEGMENT
    within r, nearest first: entries[i * k .. i * k + k - 1] (NEAREST_ENTRY_DTYPE: d2, id; unused slots d2 = r * r, id -1) and / or records (k
    SEGMENT_RECORD_DTYPE records per query: q on the triangle, d2, id, feature 0 .. 4, side, s on the segment); one of the two may be 0.
    1 <= k <= MAX_NEAREST; cursors and paging as nearest_tris.  query_labels (int32[2 n]: an edge's two vertex indices, -1 unused) and tri_labels
    (int32[3 per scene triangle]): both or neither; a triangle that carries one of the query's labels (>= 0) is left out (MeshScene.edge_labels: an
    edge does not see the triangles that share a vertex with it).  counters: 0, or a device int64[5] as nearest_tris.  All arguments are device
    addresses (a torch tensor passes as t.data_ptr()); asynchronous on the manager's stream.  scene.segment_tris states the results in numpy, bit for
    bit.  Walks the construction format: not for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_segment_tris(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(segments or 0), int(n), int(k), C.c_void_p(cursors or 0),
                                           C.c_void_p(query_labels or 0), C.c_void_p(tri_labels or 0), C.c_void_p(entries or 0), C.c_void_p(records or 0),
                                           C.c_void_p(counters or 0), 0), "segment_tris")


def tris_near_segments(grid: Grid, tris, segments, k: int = MAX_NEAREST, query_labels=None, tri_labels=None, max_pages=None) -> dict:
    """ALL the triangles within r of every segment, nearest first, in CSR form: segment_tris paged on torch tensors, the analogue of tris_within
    (the same keys, the same cost model, the same use of the fifth counter).  segments ((n, 8) float32: ax, ay, az, r, bx, by, bz, 0), query_labels
    ((n, 2) int32) and tri_labels ((N, 3) int32): torch tensors on the device (tris and tri_labels may be device addresses).  What scene.tris_near_segments
    states.  For finite radii."""
    return _paged_csr(segment_tris, 8, grid, tris, segments, k, query_labels, tri_labels, max_pages)


MAX_OVERLAP_IDS = 8      # HAGRID_MAX_OVERLAP_IDS
OVERLAP_ANY = 1          # HAGRID_OVERLAP_ANY


def overlap_boxes(grid: Grid, tris: int, boxes: int, n: int, k: int, ids: int, counts: int = 0, counters: int = 0, flags: int = 0):
    """Extension (hagrid_overlap_boxes): for each of n boxes (32 bytes: BOX_QUERY_DTYPE -- min, first, max, pad) the k smallest ids >= first of the
    triangles that meet it, ascending, into ids[i * k .. i * k + k - 1] (int32, unused slots -1), and min(how many meet it, k + 1) into counts[i] (int32;
    counts may be 0).  1 <= k <= MAX_OVERLAP_IDS; flags: 0 | OVERLAP_ANY (k = 1: stop at the first triangle that meets the box).  counters: 0, or a device
    int64[4] the batch totals are added to (boxes, cells visited, triangle / box tests, sub-blocks pruned).  All arguments are device addresses (a torch
    tensor passes as t.data_ptr()); asynchronous on the manager's stream.  Every box is clipped to the grid box first, so infinite bounds mean "no bound on
    this side".  ids: 16-byte aligned for k = 4 and k = 8, 4-byte aligned otherwise.  scene.overlap_boxes states the results in numpy.  Walks the construction
    format: not for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_overlap_boxes(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(boxes or 0), int(n), int(k), C.c_void_p(ids or 0),
                                            C.c_void_p(counts or 0), C.c_void_p(counters or 0), int(flags)), "overlap_boxes")


def voxelize(grid: Grid, tris: int, origin, size, n, k: int, ids: int, counts: int = 0, counters: int = 0, flags: int = 0):
    """Extension (hagrid_overlap_lattice): overlap_boxes over the voxels of an n[0] x n[1] x n[2] lattice, x fastest, made on the device: voxel c of an
    axis is [origin + float(c) * size, origin + float(c + 1) * size] (scene.lattice_boxes gives the same boxes).  origin, size: 3 floats, n: 3 ints (host
    values); ids: n[0] * n[1] * n[2] * k int32 on the device.  With k = 1 and OVERLAP_ANY, ids >= 0 is the surface voxelization of the mesh."""
    mem = grid.mem or _current
    o = (C.c_float * 3)(*[float(v) for v in origin]); s = (C.c_float * 3)(*[float(v) for v in size]); m = (C.c_int * 3)(*[int(v) for v in n])
    _check(mem, mem._L.hagrid_overlap_lattice(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), o, s, m, int(k), C.c_void_p(ids or 0), C.c_void_p(counts or 0),
                                              C.c_void_p(counters or 0), int(flags)), "voxelize")


def overlap_tris(grid: Grid, tris: int, queries: int, n: int, k: int, ids: int, counts: int = 0, counters: int = 0, flags: int = 0, first: int = 0,
                 query_labels: int = 0, tri_labels: int = 0):
    """Extension (hagrid_overlap_tris): CONTACT queries -- for each of n query triangles (48-byte Tri records) the k smallest ids >= first[i] of the scene
    triangles it touches, into ids and counts exactly as overlap_boxes writes them (ANY likewise).  Two triangles touch when no axis of the separating-axis
    test separates them (include/hagrid/tri_tri.h; scene.tri_tri_pairs) and the scene triangle meets the query's bounding box grown by the grid's margin.
    first: 0, or a device int32[n].  query_labels (int32[3 n]) and tri_labels (int32[3 per scene triangle]): both or neither; a pair that shares a label
    >= 0 is left out -- a mesh's index triples (MeshScene.vertex_labels) leave out the triangle itself and every neighbour that shares a vertex, body ids
    the contacts inside one body.  Scene triangles with a stored normal of 0 take no part; a query that is not finite or has a stored normal of 0 gets
    count 0.  `queries` may be `tris`.  counters: as for overlap_boxes; the third total counts the pairs offered to the triangle / triangle test.  All
    arguments are device addresses; asynchronous on the manager's stream.  scene.overlap_tris states the results in numpy.  Walks the construction
    format: not for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_overlap_tris(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(queries or 0), int(n), C.c_void_p(first or 0),
                                           C.c_void_p(query_labels or 0), C.c_void_p(tri_labels or 0), int(k), C.c_void_p(ids or 0), C.c_void_p(counts or 0),
                                           C.c_void_p(counters or 0), int(flags)), "overlap_tris")


def self_intersections(grid: Grid, tris, labels, k: int = MAX_OVERLAP_IDS):
    """The triangles of a scene that touch each other though they are no neighbours: overlap_tris with the scene's own triangles as queries, `labels` for
    both sides and first[i] = i + 1, so every pair is reported once, at its smaller id.  tris: a torch float32 tensor (N, 12) on the device, the array the
    grid was built over; labels: a torch int32 tensor (N, 3) (MeshScene.vertex_labels).  Returns (ids (N, k) int32, counts (N,) int32) as torch tensors;
    counts[i] = k + 1 says "more": ask overlap_tris again with first = ids[i, k - 1] + 1."""
    import torch
    mem = grid.mem or _current
    n = int(tris.shape[0])
    with torch.cuda.stream(mem.torch_stream()):
        first = torch.arange(1, n + 1, dtype=torch.int32, device=tris.device)
        ids = torch.empty((n, int(k)), dtype=torch.int32, device=tris.device)
        counts = torch.empty((n,), dtype=torch.int32, device=tris.device)
        overlap_tris(grid, tris.data_ptr(), tris.data_ptr(), n, k, ids.data_ptr(), counts.data_ptr(), first=first.data_ptr(), query_labels=labels.data_ptr(),
                     tri_labels=labels.data_ptr())
    return ids, counts


def overlap_obbs(grid: Grid, tris: int, obbs: int, n: int, k: int, ids: int, counts: int = 0, counters: int = 0, flags: int = 0, query_labels: int = 0,
                 tri_labels: int = 0):
    """Extension (hagrid_overlap_obbs): ORIENTED-BOX queries -- for each of n boxes (64 bytes: OBB_DTYPE -- c, first, u, 0, v, 0, w, 0; the box is
    c + a u + b v + g w with |a|, |b|, |g| <= 1, the axes neither normalised nor orthogonal) the k smallest ids >= first of the scene triangles that meet it,
    into ids and counts exactly as overlap_boxes writes them (ANY likewise).  A triangle meets the box when no axis of the separating-axis test separates
    them (include/hagrid/obb.h; scene.obb_pairs) and it meets the box's bounding box grown by the grid's margin.  query_labels (int32[n], one per box) and
    tri_labels (int32[3 per scene triangle]): both or neither; a pair is left out when the box's label is >= 0 and one of the triangle's three -- with
    body ids a body's box does not see the body's own triangles.  A record with a component that is not finite gets count 0.  counters: as for
    overlap_boxes; the third total counts the pairs offered to the box / triangle test.  All arguments are device addresses; asynchronous on the manager's
    stream.  scene.overlap_obbs states the results in numpy.  Walks the construction format: not for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_overlap_obbs(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(obbs or 0), int(n), C.c_void_p(query_labels or 0),
                                           C.c_void_p(tri_labels or 0), int(k), C.c_void_p(ids or 0), C.c_void_p(counts or 0), C.c_void_p(counters or 0), int(flags)),
           "overlap_obbs")


def obb_records(centres, rotations_or_axes, half_extents=None, first=None):
    """OBB records for overlap_obbs from torch tensors on the device: a float32 tensor (n, 16).  centres (n, 3); rotations_or_axes (n, 3, 3) whose COLUMNS
    are the directions of the box's three axes (a rotation matrix, or any frame -- a sheared one is legal); half_extents (n, 3) scales the columns, None
    takes them as they are (u, v, w themselves).  first: None (0) or an int32 tensor (n,).  Runs on torch's current stream."""
    import torch
    c = centres.to(torch.float32).reshape(-1, 3)
    A = rotations_or_axes.to(torch.float32).reshape(-1, 3, 3)
    if half_extents is not None:
        A = A * half_extents.to(torch.float32).reshape(-1, 1, 3)
    rec = torch.zeros((c.shape[0], 4, 4), dtype=torch.float32, device=c.device)
    rec[:, 0, :3] = c
    rec[:, 1:, :3] = A.transpose(1, 2)
    if first is not None:
        rec[:, 0, 3] = first.to(torch.int32).reshape(-1).view(torch.float32)
    return rec.reshape(-1, 16)


def tris_in_obbs(grid: Grid, tris, obbs, k: int = MAX_OVERLAP_IDS, query_labels=None, tri_labels=None, max_pages=None) -> dict:
    """ALL the triangles that meet every oriented box, ascending by id, in CSR form: overlap_obbs paged on torch tensors.  Page by page the boxes whose
    count came back k + 1 are asked again with first = last id + 1; ONE scalar per page goes to the host (how many lists go on).  obbs: a float32 tensor
    (n, 16) on the device (obb_records; its `first` words are respected and left unchanged), query_labels ((n,) int32) and tri_labels ((N, 3) int32): torch
    tensors on the device (tris and tri_labels may be device addresses).  The manager must run on torch's current stream.  Returns "offsets" int64
    (n + 1,), "ids" int32 (total,), "pages" and "complete" (False only when max_pages ended the paging early; the lists are then prefixes).  _paged_csr
    serves the cursor-paged distance lists and does not fit: here a page is continued by `first` inside the record, and the entries carry no distance."""
    import torch
    ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
    k = int(k)
    rec = obbs.reshape(-1, 16).clone()
    n = int(rec.shape[0])
    dev = rec.device
    active = torch.arange(n, dtype=torch.int64, device=dev)
    lab = query_labels
    page_q, page_ids = [], []
    pages, complete = 0, True
    while active.numel():
        if max_pages is not None and pages >= int(max_pages):
            complete = False
            break
        pages += 1
        m = int(active.numel())
        ids = torch.empty((m, k), dtype=torch.int32, device=dev)
        counts = torch.empty((m,), dtype=torch.int32, device=dev)
        overlap_obbs(grid, ptr(tris), rec.data_ptr(), m, k, ids.data_ptr(), counts.data_ptr(), query_labels=ptr(lab) if query_labels is not None else 0,
                     tri_labels=ptr(tri_labels) if query_labels is not None else 0)
        page_q.append(active); page_ids.append(ids)
        more = counts > k
        if int(more.sum().item()) == 0:
            break
        active = active[more]
        rec = rec[more].contiguous()
        rec[:, 3] = (ids[more][:, k - 1] + 1).view(torch.float32)
        if query_labels is not None:
            lab = lab[more].contiguous()
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if not page_q:
        return {"offsets": offsets, "ids": torch.zeros(0, dtype=torch.int32, device=dev), "pages": 0, "complete": complete}
    q = torch.cat([a[:, None].expand(-1, k).reshape(-1) for a in page_q])
    e = torch.cat([x.reshape(-1) for x in page_ids])
    used = e >= 0
    q, e = q[used], e[used]
    e = e[torch.sort(q, stable=True)[1]]
    torch.cumsum(torch.bincount(q, minlength=n), 0, out=offsets[1:])
    return {"offsets": offsets, "ids": e.contiguous(), "pages": pages, "complete": complete}


# ---- overlap lists: ALL of every region query's answer in one pass (hagrid_box_refs, hagrid_tri_refs, hagrid_obb_refs) -------------

def box_refs(grid: Grid, tris: int, boxes: int, n: int, counts: int = 0, offsets: int = 0, entries: int = 0, capacity: int = 0, counters: int = 0):
    """Extension (hagrid_box_refs): stage 1 of the OVERLAP LISTS for boxes -- the walk of overlap_boxes with a list that keeps nothing.  A REFERENCE is one
    triangle >= first that meets the box, as the walk meets it; a triangle arrives once per visit of a cell that lists it, so references hold duplicates.
    Count mode (offsets = 0, entries = 0, capacity = 0): counts[i] (int32[n]) = R_i, the references of box i.  Fill mode: offsets int64[n + 1] -- box i owns
    the slots [offsets[i], offsets[i + 1]) of `entries` (capacity slots of NEAREST_ENTRY_DTYPE) and writes its first min(R_i, room) references in walk order
    as (+0.0, id), then the empty entry (+inf, -1); the room rule is list_crossings'.  counters: 0, or a device int64[6] added to (boxes, cells visited,
    triangle / box tests, sub-blocks pruned, references written, boxes that did not fit).  unique_lists and compact_lists make the lists of it.  Device
    addresses; asynchronous on the manager's stream.  Walks the construction format: not for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_box_refs(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(boxes or 0), int(n), C.c_void_p(offsets or 0), C.c_void_p(counts or 0),
                                       C.c_void_p(entries or 0), int(capacity), C.c_void_p(counters or 0), 0), "box_refs")


def tri_refs(grid: Grid, tris: int, queries: int, n: int, counts: int = 0, offsets: int = 0, entries: int = 0, capacity: int = 0, first: int = 0, query_labels: int = 0,
             tri_labels: int = 0, counters: int = 0):
    """Extension (hagrid_tri_refs): stage 1 of the OVERLAP LISTS for contact queries -- box_refs with the queries, first and labels of overlap_tris; the
    third counter counts the pairs offered to the triangle / triangle test."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_tri_refs(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(queries or 0), int(n), C.c_void_p(first or 0), C.c_void_p(query_labels or 0),
                                       C.c_void_p(tri_labels or 0), C.c_void_p(offsets or 0), C.c_void_p(counts or 0), C.c_void_p(entries or 0), int(capacity),
                                       C.c_void_p(counters or 0), 0), "tri_refs")


def obb_refs(grid: Grid, tris: int, obbs: int, n: int, counts: int = 0, offsets: int = 0, entries: int = 0, capacity: int = 0, query_labels: int = 0, tri_labels: int = 0,
             counters: int = 0):
    """Extension (hagrid_obb_refs): stage 1 of the OVERLAP LISTS for oriented boxes -- box_refs with the records and labels of overlap_obbs; the third counter
    counts the pairs offered to the box / triangle test."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_obb_refs(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(obbs or 0), int(n), C.c_void_p(query_labels or 0),
                                       C.c_void_p(tri_labels or 0), C.c_void_p(offsets or 0), C.c_void_p(counts or 0), C.c_void_p(entries or 0), int(capacity),
                                       C.c_void_p(counters or 0), 0), "obb_refs")


def _label_pair(who: str, ptr, query_labels, tri_labels):
    """the device addresses of the two label arrays, (0, 0) for none; one without the other is refused here as the entry points refuse it"""
    if (query_labels is None) != (tri_labels is None):
        raise HagridError(f"{who}: query_labels and tri_labels are given together or not at all")
    return (ptr(query_labels), ptr(tri_labels)) if query_labels is not None else (0, 0)


def _overlap_lists(mem, n: int, dev, refs_stage) -> dict:
    """the protocol of ball_lists with refs_stage(counts, offsets, entries, capacity) as stage 1: count, torch.cumsum, fill, unique_lists, torch.cumsum,
    compact_lists; TWO scalars go to the host (the totals that size the scratch and the output)"""
    import torch
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    refs_stage(counts.data_ptr(), 0, 0, 0)
    ref_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum(counts, 0, dtype=torch.int64, out=ref_offsets[1:])
    refs = int(ref_offsets[-1].item())
    scratch = torch.empty((refs, 2), dtype=torch.int32, device=dev)
    refs_stage(0, ref_offsets.data_ptr(), scratch.data_ptr() if refs else 0, refs)
    unique_lists(n, ref_offsets.data_ptr(), scratch.data_ptr() if refs else 0, refs, counts.data_ptr(), mem=mem)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    total = int(offsets[-1].item())
    out = torch.empty((total, 2), dtype=torch.int32, device=dev)
    compact_lists(n, ref_offsets.data_ptr(), scratch.data_ptr() if refs else 0, refs, counts.data_ptr(), offsets.data_ptr(), out.data_ptr() if total else 0, total, mem=mem)
    return {"offsets": offsets, "ids": out[:, 1].contiguous(), "refs": refs}


def box_lists(grid: Grid, tris, boxes) -> dict:
    """ALL the triangles that meet every box, ascending by id, in CSR form, WITHOUT paging: box_refs (count), torch.cumsum, box_refs (fill), unique_lists,
    torch.cumsum, compact_lists on torch tensors; TWO scalars go to the host.  boxes: a float32 tensor (n, 8) on the device (BOX_QUERY_DTYPE rows; `first` is
    respected); tris: a tensor or a device address.  The manager must run on torch's current stream.  Returns "offsets" int64 (n + 1,), "ids" int32 (total,)
    -- what scene.box_lists states, and what paging overlap_boxes to the end concatenates to -- and "refs", the total of R_i: the scratch (8 bytes each) a
    caller of the staged entry points needs.  Linear in the list where paging is quadratic."""
    ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
    rec = boxes.reshape(-1, 8)
    n = int(rec.shape[0])
    return _overlap_lists(grid.mem or _current, n, rec.device,
                          lambda counts, offsets, entries, capacity: box_refs(grid, ptr(tris), rec.data_ptr(), n, counts=counts, offsets=offsets, entries=entries, capacity=capacity))


def contact_lists(grid: Grid, tris, queries, first=None, query_labels=None, tri_labels=None) -> dict:
    """ALL the scene triangles every query triangle touches, ascending by id, in CSR form, WITHOUT paging: the protocol of box_lists over tri_refs.  queries: a
    float32 tensor (n, 12) on the device (may be the scene's own array); first ((n,) int32), query_labels ((n, 3) int32) and tri_labels ((N, 3) int32): torch
    tensors on the device or None, the labels both or neither (tris and tri_labels may be device addresses).  Returns what box_lists returns; what
    scene.contact_lists states.  contact_lists(grid, tris, tris, first=arange(1, N + 1), query_labels=labels, tri_labels=labels) gives ALL self-intersections
    of a mesh, each pair once, at its smaller id -- self_intersections without the bound k."""
    ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
    rec = queries.reshape(-1, 12)
    n = int(rec.shape[0])
    ql, tl = _label_pair("contact_lists", ptr, query_labels, tri_labels)
    return _overlap_lists(grid.mem or _current, n, rec.device,
                          lambda counts, offsets, entries, capacity: tri_refs(grid, ptr(tris), rec.data_ptr(), n, counts=counts, offsets=offsets, entries=entries, capacity=capacity,
                                                                              first=ptr(first) if first is not None else 0, query_labels=ql, tri_labels=tl))


def obb_lists(grid: Grid, tris, obbs, query_labels=None, tri_labels=None) -> dict:
    """ALL the triangles that meet every oriented box, ascending by id, in CSR form, WITHOUT paging: the protocol of box_lists over obb_refs.  Arguments as
    tris_in_obbs, whose "offsets" and "ids" these are; what scene.obb_lists states."""
    ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
    rec = obbs.reshape(-1, 16)
    n = int(rec.shape[0])
    ql, tl = _label_pair("obb_lists", ptr, query_labels, tri_labels)
    return _overlap_lists(grid.mem or _current, n, rec.device,
                          lambda counts, offsets, entries, capacity: obb_refs(grid, ptr(tris), rec.data_ptr(), n, counts=counts, offsets=offsets, entries=entries, capacity=capacity,
                                                                              query_labels=ql, tri_labels=tl))


INSIDE_WINDING = 1       # HAGRID_INSIDE_WINDING


def _dirs(dirs):
    """(pointer or None, num_dirs) of the host directions of points_inside / inside_lattice: None = the three defaults (scene.CROSSING_DIRS)"""
    if dirs is None:
        return None, 0
    import numpy as np
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    return (C.c_float * d.size)(*[float(v) for v in d.reshape(-1)]), d.shape[0]


def count_crossings(grid: Grid, tris: int, rays: int, records: int, num_rays: int, counters: int = 0, flags: int = 0):
    """Extension (hagrid_count_crossings): for each of num_rays rays ALL the triangles it crosses (the intersections of traverse_grid_multi, without the
    bound k), condensed into one Hit-shaped record (HIT_DTYPE): id = count, t = the first t (the bits of tmax when there is none), u = length = the sum of
    t[2p+1] - t[2p] over the pairs in (t, id) order, v = the int32 bits of winding = #leaving - #entering.  counters: 0, or a device int64[4] the batch
    totals are added to (rays, cells visited, triangle tests, pages flushed).  All arguments are device addresses (a torch tensor passes as
    t.data_ptr()); asynchronous on the manager's stream.  scene.ray_crossings states the records in numpy, bit for bit.  Walks the construction format: not
    for a grid given up with release_for_traversal."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_count_crossings(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(rays or 0), C.c_void_p(records or 0), int(num_rays),
                                              C.c_void_p(counters or 0), int(flags)), "count_crossings")


def list_crossings(grid: Grid, tris: int, rays: int, num_rays: int, entries: int, capacity: int, offsets: int = 0, stride: int = 0, records: int = 0, counters: int = 0):
    """Extension (hagrid_list_crossings): the crossings of count_crossings THEMSELVES, sorted by (t, id), 8 bytes each: float32 t; int32 key = id * 2 + entering.
    offsets: a device int64[num_rays + 1] -- ray i owns the slots [offsets[i], offsets[i+1]) of `entries` (capacity slots) -- or 0 with stride = S >= 1: ray i owns
    [i * S, (i + 1) * S).  A ray writes its first min(m, room) entries and fills the rest of its slots with the empty entry (the bits of tmax, -1); a pair of
    offsets that is negative, decreasing or beyond the capacity has room 0.  records: 0, or the records of count_crossings (record.id > room: the list did not
    fit); counters: 0, or a device int64[6] added to (rays, cells, tests, flushes, entries written, rays that did not fit).  Device addresses; asynchronous on
    the manager's stream.  scene.ray_crossing_lists and scene.crossing_slots state it in numpy."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_list_crossings(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(rays or 0), int(num_rays), C.c_void_p(offsets or 0), int(stride),
                                             C.c_void_p(entries or 0), int(capacity), C.c_void_p(records or 0), C.c_void_p(counters or 0), 0), "list_crossings")


def crossing_lists(grid: Grid, tris, rays, num_rays: int) -> dict:
    """count, scan, fill on torch tensors: count_crossings, torch.cumsum of the counts into int64 offsets, ONE scalar to the host (the total, which sizes the
    output), list_crossings.  tris, rays: torch tensors on the device (or device addresses).  The manager must run on torch's current stream
    (mem.use_stream(torch.cuda.current_stream().cuda_stream)).  Returns "offsets" int64 (n + 1,), "t" float32, "tri" int32 and "entering" bool (total,): the
    crossings of ray i are offsets[i] .. offsets[i+1], sorted by (t, id); "entries" int32 (total, 2), the raw words (t is a view of it), and "records" int32
    (n, 4): count, the bits of t_first, the bits of length, winding."""
    import torch
    n = int(num_rays)
    ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
    dev = rays.device if hasattr(rays, "device") else torch.device("cuda", torch.cuda.current_device())
    records = torch.empty((n, 4), dtype=torch.int32, device=dev)
    count_crossings(grid, ptr(tris), ptr(rays), records.data_ptr(), n)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum(records[:, 0], 0, dtype=torch.int64, out=offsets[1:])
    total = int(offsets[-1].item())
    entries = torch.empty((total, 2), dtype=torch.int32, device=dev)
    list_crossings(grid, ptr(tris), ptr(rays), n, entries.data_ptr() if total else 0, total, offsets=offsets.data_ptr())
    return {"offsets": offsets, "t": entries.view(torch.float32)[:, 0], "tri": entries[:, 1] >> 1, "entering": (entries[:, 1] & 1) != 0, "entries": entries,
            "records": records}


def points_inside(grid: Grid, tris: int, points: int, n: int, inside: int, dirs=None, records: int = 0, counters: int = 0, flags: int = 0):
    """Extension (hagrid_points_inside): for each of n points (16 bytes: x, y, z, reach -- POINT_QUERY_DTYPE) whether it lies inside the closed surface the
    triangles form: a ray per direction (dirs: None = the three of scene.CROSSING_DIRS, or 1 or 3 host directions) from the point to `reach` (+inf: no
    bound), the vote of a ray is count & 1 (flags INSIDE_WINDING: winding != 0), inside[i] (int32) = 1 when most rays vote inside, else 0; -1 for an
    inactive point (reach < 0 or NaN, a NaN or infinite coordinate).  records: 0, or n * m Hit-shaped records (direction fastest) for the per-ray records
    of count_crossings.  scene.points_inside states the results in numpy."""
    mem = grid.mem or _current
    d, m = _dirs(dirs)
    _check(mem, mem._L.hagrid_points_inside(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), C.c_void_p(points or 0), int(n), d, int(m), C.c_void_p(inside or 0),
                                            C.c_void_p(records or 0), C.c_void_p(counters or 0), int(flags)), "points_inside")


def inside_lattice(grid: Grid, tris: int, origin, size, n, inside: int, dirs=None, records: int = 0, counters: int = 0, flags: int = 0):
    """Extension (hagrid_inside_lattice): points_inside over the voxel centres of an n[0] x n[1] x n[2] lattice, x fastest, made on the device: the centre of
    voxel c of an axis is origin + (float(c) + 0.5) * size (scene.lattice_centres gives the same points), reach +inf.  origin, size: 3 floats, n: 3 ints
    (host values); inside: n[0] * n[1] * n[2] int32 on the device.  Together with voxelize (the voxels the surface meets) this is the solid voxelization."""
    mem = grid.mem or _current
    o = (C.c_float * 3)(*[float(v) for v in origin]); s = (C.c_float * 3)(*[float(v) for v in size]); k = (C.c_int * 3)(*[int(v) for v in n])
    d, m = _dirs(dirs)
    _check(mem, mem._L.hagrid_inside_lattice(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), o, s, k, d, int(m), C.c_void_p(inside or 0), C.c_void_p(records or 0),
                                             C.c_void_p(counters or 0), int(flags)), "inside_lattice")


def fill_lattice(grid: Grid, tris: int, origin, size, n, inside: int, axes: int = 7, workspace: int = 0, records: int = 0, counters: int = 0, flags: int = 0):
    """Extension (hagrid_fill_lattice): the inside of a closed surface on the lattice of inside_lattice by scan lines -- ONE ray per voxel row of every axis in
    `axes` (1 = x, 2 = y, 4 = z; 0 means 7) instead of one to three per voxel.  A row's vote for voxel c is its state over the crossings before the voxel's centre
    (count & 1; flags INSIDE_WINDING, the recommended rule: leaving minus entering != 0); a row that ends inside abstains; inside (int32 per voxel, x fastest) is 1
    when most usable rows vote inside, else 0, -1 where no row was usable.  workspace: one byte per voxel on the device, needed with more than one axis.  records:
    0, or the records of the row rays (count_crossings), axis after axis; counters: 0, or a device int64[5] added to (rows, cells, tests, flushes, rows that
    abstained).  Device addresses; asynchronous on the manager's stream.  scene.fill_lattice states the results in numpy."""
    mem = grid.mem or _current
    o = (C.c_float * 3)(*[float(v) for v in origin]); s = (C.c_float * 3)(*[float(v) for v in size]); k = (C.c_int * 3)(*[int(v) for v in n])
    _check(mem, mem._L.hagrid_fill_lattice(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), o, s, k, int(axes), C.c_void_p(inside or 0), C.c_void_p(workspace or 0),
                                           C.c_void_p(records or 0), C.c_void_p(counters or 0), int(flags)), "fill_lattice")


def solid_voxels(grid: Grid, tris, origin, size, n, axes: int = 7, winding: bool = True):
    """The solid voxelization of a closed surface: fill_lattice on torch's current stream (the manager must run on it: mem.use_stream(
    torch.cuda.current_stream().cuda_stream)), the workspace allocated here.  tris: a torch tensor on the device (or a device address).  Returns a torch.int32
    tensor of shape (nz, ny, nx): 1 inside, 0 outside, -1 where no row was usable."""
    import torch
    nx, ny, nz = (int(v) for v in n)
    dev = tris.device if hasattr(tris, "device") else torch.device("cuda", torch.cuda.current_device())
    inside = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
    work = torch.empty(nx * ny * nz, dtype=torch.uint8, device=dev)
    fill_lattice(grid, tris.data_ptr() if hasattr(tris, "data_ptr") else int(tris or 0), origin, size, (nx, ny, nz), inside.data_ptr(), axes=axes, workspace=work.data_ptr(),
                 flags=INSIDE_WINDING if winding else 0)
    return inside


def distance_lattice(grid: Grid, tris: int, origin, size, n, band: float, workspace: int, ids: int = 0, d2: int = 0, records: int = 0, counters: int = 0):
    """Extension (hagrid_distance_lattice): closest_points over the voxel centres of the lattice of inside_lattice with r = band (finite, >= 0), made by scatter:
    every triangle visits the voxels within the band of it and takes the minimum into the voxel's slot.  workspace: 8 bytes per voxel on the device (initialised
    by the call); ids (int32), d2 (float32), records (CLOSEST_DTYPE, 32 bytes): one per voxel, x fastest, each may be 0 but not all three.  Nothing within the band:
    id -1, d2 = band * band, q = the centre.  counters: 0, or a device int64[4] added to (triangles with a voxel box, tasks, pairs within the band, voxels with an
    answer).  Device addresses; on the manager's stream.  scene.distance_lattice states the results in numpy, bit for bit."""
    mem = grid.mem or _current
    o = (C.c_float * 3)(*[float(v) for v in origin]); s = (C.c_float * 3)(*[float(v) for v in size]); k = (C.c_int * 3)(*[int(v) for v in n])
    _check(mem, mem._L.hagrid_distance_lattice(mem._ctx, C.byref(grid.pod), C.c_void_p(tris or 0), o, s, k, C.c_float(float(band)), C.c_void_p(workspace or 0),
                                               C.c_void_p(ids or 0), C.c_void_p(d2 or 0), C.c_void_p(records or 0), C.c_void_p(counters or 0), 0), "distance_lattice")


def signed_distance_lattice(grid: Grid, tris, origin, size, n, band: float, axes: int = 7) -> dict:
    """A narrow-band signed distance field of a closed surface on the lattice: distance_lattice for the magnitude and fill_lattice (winding rule) for the sign, on
    torch's current stream (the manager must run on it: mem.use_stream(torch.cuda.current_stream().cuda_stream)), the workspaces allocated here.  tris: a torch
    tensor on the device (or a device address).  Returns torch tensors of shape (nz, ny, nx): "sdf" float32 = sqrt(d2), negative where inside == 1, so +-band where
    no triangle lies within the band; "d2" float32; "ids" int32 (-1: none); "inside" int32 (1, 0, or -1 where no row was usable: such voxels keep the positive
    sign).  The sign is fill_lattice's: not robust for centres ON the surface."""
    import torch
    nx, ny, nz = (int(v) for v in n)
    dev = tris.device if hasattr(tris, "device") else torch.device("cuda", torch.cuda.current_device())
    d_tris = tris.data_ptr() if hasattr(tris, "data_ptr") else int(tris or 0)
    ids = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
    d2 = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    inside = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
    slots = torch.empty(nx * ny * nz, dtype=torch.int64, device=dev)
    work = torch.empty(nx * ny * nz, dtype=torch.uint8, device=dev)
    distance_lattice(grid, d_tris, origin, size, (nx, ny, nz), band, slots.data_ptr(), ids=ids.data_ptr(), d2=d2.data_ptr())
    fill_lattice(grid, d_tris, origin, size, (nx, ny, nz), inside.data_ptr(), axes=axes, workspace=work.data_ptr(), flags=INSIDE_WINDING)
    sdf = torch.sqrt(d2)
    sdf = torch.where(inside == 1, -sdf, sdf)
    return {"sdf": sdf, "d2": d2, "ids": ids, "inside": inside}


def traverse_grid_stats(grid: Grid, tris: int, rays: int, hits: int, num_rays: int, steps: int = 0) -> dict:
    mem = grid.mem or _current
    st = TraversalStats()
    _check(mem, mem._L.hagrid_traverse_grid_stats(mem._ctx, C.byref(grid.pod), C.c_void_p(tris), C.c_void_p(rays), C.c_void_p(hits),
                                                  int(num_rays), C.c_void_p(steps), C.byref(st)), "traverse_grid_stats")
    return st.as_dict()


# ---- frames on the device (include/hagrid_amd.h "frames on the device", include/hagrid/frame.h) ----------------------------

SHADE_DEPTH, SHADE_GRAY, SHADE_HEAT = 0, 1, 2      # hagrid_shade_hits / hagrid_render_frame modes
BOUNCE_REDRAW_MISSES = 1                           # hagrid_gen_bounce_rays flag


def _camera(cam) -> Camera:
    return cam if isinstance(cam, Camera) else Camera.from_scene(cam)


def _f3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


def gen_primary_rays(mem: MemManager, cam, clip: float, width: int, height: int, rays: int, first: int = 0, count: int | None = None):
    """gen_rays (main.cpp:52-66) on the device: the rays of pixels first .. first+count-1 into `rays` (32 bytes each); the bits of
    scene.make_rays_primary.  cam: a Camera or the tuple scene.camera returns."""
    if count is None:
        count = width * height - first
    _check(mem, mem._L.hagrid_gen_primary_rays(mem._ctx, C.byref(_camera(cam)), float(clip), int(width), int(height), int(first), int(count), C.c_void_p(rays)), "gen_primary_rays")


def gen_bounce_rays(mem: MemManager, tris: int, rays: int, hits: int, num_rays: int, seed: int, bbox_min, bbox_max, out_rays: int,
                    first: int = 0, tmax: float = 3.4028234663852886e38, redraw_misses: bool = True):
    """scene.make_rays_bounce on the device (same bits): from rays and their hits to diffuse-bounce rays in `out_rays`."""
    _check(mem, mem._L.hagrid_gen_bounce_rays(mem._ctx, C.c_void_p(tris), C.c_void_p(rays), C.c_void_p(hits), int(num_rays), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              int(first), _f3(bbox_min), _f3(bbox_max), float(tmax), BOUNCE_REDRAW_MISSES if redraw_misses else 0, C.c_void_p(out_rays)), "gen_bounce_rays")


def shade_hits(mem: MemManager, hits: int, num_hits: int, mode: int, clip: float, bgra: int):
    """update_surface (main.cpp:90-111) on the device: 4 bytes per pixel (B G R A) into `bgra`; scene.shade_hits states the formulas."""
    _check(mem, mem._L.hagrid_shade_hits(mem._ctx, C.c_void_p(hits), int(num_hits), int(mode), float(clip), C.c_void_p(bgra)), "shade_hits")


def shade_layers(mem: MemManager, hits: int, num_rays: int, k: int, clip: float, opacity: float, bgra: int):
    """The layered picture of the hit lists of traverse_grid_multi (k records per pixel) on the device: every surface a layer of the given
    opacity in its depth colour, front to back over white; scene.shade_layers states the formula."""
    _check(mem, mem._L.hagrid_shade_layers(mem._ctx, C.c_void_p(hits), int(num_rays), int(k), float(clip), float(opacity), C.c_void_p(bgra)), "shade_layers")


def accumulate_occlusion(mem: MemManager, occlusion_hits: int, num_rays: int, counts: int):
    """counts[i] += occlusion_hits[i].id >= 0 (int32 per ray)."""
    _check(mem, mem._L.hagrid_accumulate_occlusion(mem._ctx, C.c_void_p(occlusion_hits), int(num_rays), C.c_void_p(counts)), "accumulate_occlusion")


def shade_occlusion(mem: MemManager, hits: int, counts: int, num_rays: int, samples: int, bgra: int):
    """The ambient-occlusion picture of primary hits and their occlusion counts (scene.shade_occlusion)."""
    _check(mem, mem._L.hagrid_shade_occlusion(mem._ctx, C.c_void_p(hits), C.c_void_p(counts), int(num_rays), int(samples), C.c_void_p(bgra)), "shade_occlusion")


def frame_workspace_bytes(width: int, height: int, ao_samples: int = 0) -> int:
    return int(_lib.load().hagrid_frame_workspace_bytes(int(width), int(height), int(ao_samples)))


def frame_workspace_layout(width: int, height: int, ao_samples: int = 0) -> dict:
    """Byte offsets of the sections of a frame workspace, as include/hagrid_amd.h documents them: every section at the next multiple of 256."""
    n = int(width) * int(height)
    up = lambda v: (v + 255) // 256 * 256
    lay = {"rays": 0, "hits": up(32 * n)}
    total = lay["hits"] + up(16 * n)
    if ao_samples > 0:
        lay["bounce_rays"] = total
        lay["occlusion_hits"] = lay["bounce_rays"] + up(32 * n)
        lay["counts"] = lay["occlusion_hits"] + up(16 * n)
        total = lay["counts"] + up(4 * n)
    lay["total"] = total
    return lay


def render_frame(grid: Grid, tris: int, cam, clip: float, width: int, height: int, workspace: int, bgra: int, mode: int = SHADE_DEPTH,
                 ao_samples: int = 0, ao_radius: float = 0.0, seed: int = 0):
    """One frame on the manager's stream: primary rays -> traversal -> pixels (hagrid_render_frame); nothing is copied or waited for.
    workspace: frame_workspace_bytes(...) bytes of device memory; bgra: 4 * width * height bytes (e.g. a torch.uint8 tensor's data_ptr())."""
    mem = grid.mem or _current
    _check(mem, mem._L.hagrid_render_frame(mem._ctx, C.byref(grid.pod), C.c_void_p(tris), C.byref(_camera(cam)), float(clip), int(width), int(height), int(mode),
                                           int(ao_samples), float(ao_radius), int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(workspace), C.c_void_p(bgra)), "render_frame")


# ---- scenes on the device (include/hagrid_amd.h "scenes on the device", include/hagrid/assemble.h) -------------------------

class MeshScene:
    """A scene of indexed meshes and instances whose Tri array is assembled ON THE DEVICE (hagrid_scene_create / hagrid_scene_assemble): what comes
    before build_grid in a frame loop.  meshes: a list of (vertices_ptr, num_vertices, indices_ptr_or_0, num_tris[, stride = 12]) -- vertices are
    float32 x, y, z records `stride` bytes apart, indices int32 triples (0: triangle p uses vertices 3p, 3p+1, 3p+2).  instance_mesh: the mesh every
    instance places (None: one instance per mesh, in order).  scene.assemble_tris states the result in numpy, bit for bit.

    Addresses are plain integers, like everywhere in this module: a torch tensor goes in as t.data_ptr().  The scene keeps the ADDRESSES, not
    copies -- the buffers are read at every assemble(), so a simulation may rewrite the vertices in place between frames -- which means the tensors
    must stay alive (and must not be reallocated) for as long as the scene is used.  The launch runs on the manager's stream:
    mem.use_stream(torch.cuda.current_stream().cuda_stream) orders it after the torch work that wrote the tensors."""

    def __init__(self, mem: MemManager, meshes, instance_mesh=None):
        self.mem = mem
        self._scene = None
        recs = (_lib.Mesh * max(len(meshes), 1))()
        for r, m in zip(recs, meshes):
            r.vertices, r.num_vertices, r.indices, r.num_tris = (m[0] or None), int(m[1]), (m[2] or None), int(m[3])
            r.vertex_stride = int(m[4]) if len(m) > 4 else 12
        if instance_mesh is None:
            inst, n_inst = None, len(meshes)
        else:
            n_inst = len(instance_mesh)
            inst = (C.c_int32 * max(n_inst, 1))(*[int(k) for k in instance_mesh])
        h = C.c_void_p()
        _check(mem, mem._L.hagrid_scene_create(mem._ctx, recs, len(meshes), inst, n_inst, C.byref(h)), "scene_create")
        self._scene = h
        self._meshes = [(int(m[1]), int(m[2] or 0), int(m[3])) for m in meshes]                  # (vertices, address of the indices, triangles)
        self._instance_mesh = list(range(len(meshes))) if instance_mesh is None else [int(k) for k in instance_mesh]
        self.num_instances = n_inst
        self.num_tris = self.first_tri(n_inst)

    def first_tri(self, instance: int) -> int:
        """First output triangle of an instance; instance = num_instances gives the total."""
        return _check(self.mem, self.mem._L.hagrid_scene_first_tri(self._scene, int(instance)), "scene_first_tri")

    def assemble(self, transforms: int, tris: int, origins: int = 0):
        """One launch on the manager's stream: transforms (12 float32 per instance, or 0) and the meshes' buffers in, num_tris Tri records (48 bytes
        each, 16-byte aligned) out; origins (or 0): int32 pairs (instance, triangle within its mesh) per output triangle."""
        _check(self.mem, self.mem._L.hagrid_scene_assemble(self.mem._ctx, self._scene, C.c_void_p(transforms or 0), C.c_void_p(tris or 0), C.c_void_p(origins or 0)), "scene_assemble")

    def vertex_labels(self):
        """The labels of the assembled triangles for overlap_tris / self_intersections: a torch int32 tensor (num_tris, 3) on the device, per triangle its
        mesh's index triple (3p, 3p + 1, 3p + 2 for a mesh without indices) plus an offset per INSTANCE -- the vertices of the instances before it -- so
        that triangles share a label exactly when they share a vertex of one instance.  Made on the device from the index buffers as they are now
        (copies and additions on the manager's stream, no host round trip).  A triangle with an index outside its mesh keeps that index: it has no
        surface and takes no part in a query."""
        import torch
        mem = self.mem
        with torch.cuda.stream(mem.torch_stream()):
            out = torch.empty((self.num_tris, 3), dtype=torch.int32, device=f"cuda:{mem.device}")
            offset = 0
            for i, k in enumerate(self._instance_mesh):
                nv, idx, nt = self._meshes[k]
                a = self.first_tri(i)
                if nt and idx:
                    mem.copy_d2d(out[a:a + nt].data_ptr(), idx, 12 * nt)
                    out[a:a + nt] += offset
                elif nt:
                    out[a:a + nt] = torch.arange(offset, offset + 3 * nt, dtype=torch.int32, device=out.device).view(nt, 3)
                offset += nv
        return out

    def edge_labels(self):
        """The unique edges of the assembled triangles for segment_tris: (pairs, labels), two torch tensors (m, 2) on the device.  labels (int32) are the
        edges' two vertex labels in the label space of vertex_labels(), smaller first, every edge once, sorted -- the query_labels of the mesh's own edges
        as segments; with vertex_labels() as tri_labels an edge does not see the triangles that share a vertex with it.  pairs (int64) are the same
        numbers as indices: the vertices of the instances in instance order, to gather the segments' ends with.  Made on the device (sort and unique on
        the manager's stream)."""
        import torch
        with torch.cuda.stream(self.mem.torch_stream()):
            L = self.vertex_labels()
            e = torch.cat([L[:, [0, 1]], L[:, [1, 2]], L[:, [2, 0]]])
            e = torch.sort(e, dim=1)[0]
            e = torch.unique(e[e[:, 0] != e[:, 1]], dim=0).contiguous()
            pairs = e.to(torch.int64)
        return pairs, e

    def instance_masks(self, masks):
        """The triangle masks of traverse_grid_filtered for the assembled triangles: masks holds one 32-bit mask per INSTANCE; returns a torch int32 tensor
        (num_tris,) on the device in which every triangle carries its instance's mask (the bits of the uint32).  Fills on the manager's stream."""
        import torch
        mem = self.mem
        masks = [int(m) & 0xFFFFFFFF for m in masks]
        if len(masks) != self.num_instances:
            raise ValueError(f"instance_masks: {len(masks)} masks for {self.num_instances} instances")
        with torch.cuda.stream(mem.torch_stream()):
            out = torch.empty((self.num_tris,), dtype=torch.int32, device=f"cuda:{mem.device}")
            for i, m in enumerate(masks):
                out[self.first_tri(i):self.first_tri(i + 1)] = m - (1 << 32) if m >= (1 << 31) else m
        return out

    def bad_indices(self) -> int:
        """Output triangles of the assemble() calls since the last query that named a vertex outside their mesh (each became the degenerate
        triangle on vertex 0); waits for the stream and resets the count."""
        n = C.c_int64(0)
        _check(self.mem, self.mem._L.hagrid_scene_bad_indices(self.mem._ctx, self._scene, C.byref(n)), "scene_bad_indices")
        return int(n.value)

    def close(self):
        if getattr(self, "_scene", None) and getattr(self.mem, "_ctx", None):
            self.mem._L.hagrid_scene_destroy(self.mem._ctx, self._scene)
        self._scene = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def profile(fn, mem: MemManager | None = None) -> float:
    """Milliseconds between two events on the manager's stream around fn() (profile.cu:5-18)."""
    mem = mem or _current
    _check(mem, mem._L.hagrid_profile_begin(mem._ctx), "profile")
    fn()
    ms = mem._L.hagrid_profile_end(mem._ctx)
    if ms < 0:
        raise HagridError("profile failed")
    return float(ms)


def build_algorithmic_bytes(bc: dict) -> dict:
    """Compulsory HBM traffic of the construction per stage, SURVEY.md 8(d) "algorithmic bytes -- build", from the sizes the
    passes recorded (MemManager.build_counts): N triangles, R0 top-level references, R_l / C_l / split_l per level, C / R / E."""
    N, R0 = bc["num_tris"], bc["top_refs"]
    build = (48 * N + 32 * N + 32 * N) + (32 * N + 8 * R0) + (R0 * (8 + 48 + 32) + 8 * R0)          # bboxes, emit, filter
    L = bc["num_levels"]
    for l in range(L):
        R_l, C_l = bc["level_refs"][l], bc["level_cells"][l]
        split_l = R_l - bc["level_kept"][l] if l + 1 < L else 0
        R_next = bc["level_refs"][l + 1] if l + 1 < L else 0
        C_next = bc["level_cells"][l + 1] if l + 1 < L else 0
        build += R_l * (12 + 8) + split_l * (8 + 48 + 32) + 8 * R_next + 32 * C_next + 2 * 4 * C_l
    R, Cc, E = bc["build_refs"], bc["build_cells"], bc["build_entries"]
    build += (8 * R + 8 * R + 32 * Cc + 4 * E) + 2 * 16 * R                                        # concat, sort
    merge = sum(c * (32 + 32) + r * (4 + 4) + 2 * 4 * E + 5 * 4 * c for c, r in zip(bc["merge_cells"], bc["merge_refs"]))
    flatten = 4 * bc["flatten_entries_in"] + 4 * bc["flatten_entries_out"]
    expand = bc["expand_passes"] * bc["expand_cells"] * (32 + 32)
    compress = (32 * bc["compress_cells"] + 16 * bc["compress_cells"] + 8 * bc["compress_refs_out"]) if bc["compressed"] else 0
    out = {"build": int(build), "merge": int(merge), "flatten": int(flatten), "expand": int(expand), "compress": int(compress)}
    out["total"] = sum(out.values())
    return out


def algorithmic_bytes(stats: dict, compressed: bool, record_bytes: int = 32) -> dict:
    """DESIGN.md / BASELINE.md section 4: bytes the algorithm must touch for a batch, from exact counters.  `record_bytes`: size of
    a traversal-image record (32, or 16 for slim records: MemManager.image_record_bytes)."""
    s_cell = 16 if compressed else 32
    walk = 4 * stats["entry_words"] + s_cell * stats["cells"]
    total = 48 * stats["rays"] + walk + 52 * stats["refs"] + 4 * stats["sentinels"]
    # what the traversal-image kernel gathers for the same walk: one record per visited cell (bounds + up to four ids inline), a
    # 48-byte triangle per test, and a 4-byte id only for lists of more than four
    image = 48 * stats["rays"] + record_bytes * stats["cells"] + 48 * stats["refs"] + 4 * stats.get("long_list_refs", 0)
    return {"B_ray": int(total), "B_walk": int(walk), "B_image": int(image), "B_image_walk": int(record_bytes * stats["cells"])}


__all__ = ["MemManager", "Grid", "build_grid", "merge_grid", "flatten_grid", "expand_grid", "compress_grid", "build_all",
           "setup_traversal", "traverse_grid", "traverse_grid_stats", "profile", "algorithmic_bytes", "build_algorithmic_bytes", "HagridError",
           "HIT_DTYPE", "CELL_DTYPE", "SMALL_CELL_DTYPE",
           "Camera", "gen_primary_rays", "gen_bounce_rays", "shade_hits", "accumulate_occlusion", "shade_occlusion", "frame_workspace_bytes",
           "frame_workspace_layout", "render_frame", "SHADE_DEPTH", "SHADE_GRAY", "SHADE_HEAT", "BOUNCE_REDRAW_MISSES",
           "traverse_grid_multi", "shade_layers", "MAX_HITS", "MeshScene",
           "traverse_grid_filtered", "skip_filters", "RAY_MASK_ALL",
           "closest_points", "POINT_QUERY_DTYPE", "CLOSEST_DTYPE", "nearest_tris", "tris_within", "ball_refs", "unique_lists", "compact_lists", "ball_lists", "MAX_NEAREST", "NEAREST_ENTRY_DTYPE", "segment_tris", "tris_near_segments", "SEGMENT_DTYPE", "SEGMENT_RECORD_DTYPE", "overlap_boxes", "box_refs", "tri_refs", "obb_refs", "box_lists", "contact_lists", "obb_lists", "voxelize", "BOX_QUERY_DTYPE", "MAX_OVERLAP_IDS", "OVERLAP_ANY",
           "overlap_tris", "self_intersections", "overlap_obbs", "obb_records", "tris_in_obbs", "OBB_DTYPE",
           "count_crossings", "list_crossings", "crossing_lists", "points_inside", "inside_lattice", "fill_lattice", "solid_voxels", "INSIDE_WINDING"]
