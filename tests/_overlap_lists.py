"""What the overlap-list tests share: the three query shapes behind one interface (the scenes, queries and fixtures of _overlap, _overlap_tris and _obb,
by import), the host program tests/cpp/overlap_lists_host.cpp as callables (the brute-force lists; the walk with RefList through the whole protocol, or in fill
mode into the caller's ranges), and the protocol on the device."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _deep_grids as D
import _host
import _obb as OB
import _overlap as V
import _overlap_tris as W
from _host import ROOT, INC, oracle_grid, oracle_grid_arrays                # names the tests use

ENTRY = scene.NEAREST_ENTRY_DTYPE
SORT_CAP = 1024                                       # kSortCap of hagrid_amd/csrc/ball_lists.hip: what a wavefront sorts in LDS
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)                # an entry no launch wrote (tests/_poison.py)
SCENES = V.SCENES
SHAPES = ("box", "contact", "obb")
SHAPE_CODE = {"box": 0, "contact": 1, "obb": 2}
RECORD_BYTES = {"box": 32, "contact": 48, "obb": 64}
FIXTURES = {"box": V.FIXTURE, "contact": W.FIXTURE, "obb": OB.FIXTURE}
PAGED = {"box": (V.PAGED, V.PAGED_FROM), "contact": (W.PAGED, W.PAGED_FROM), "obb": (OB.PAGED, OB.PAGED_FROM)}
make_tris = V.make_tris


class Batch:
    """the queries of one shape: records ((n, 8), (n, 12) float32 or (n,) OBB_DTYPE), first (contact only), query_labels, tri_labels"""
    def __init__(self, shape, records, first=None, query_labels=None, tri_labels=None):
        self.shape, self.records, self.first, self.query_labels, self.tri_labels = shape, records, first, query_labels, tri_labels
        self.n = int(np.asarray(records).shape[0])

    def rows(self) -> np.ndarray:
        """(n, words) float32"""
        return np.ascontiguousarray(self.records).view(np.float32).reshape(self.n, RECORD_BYTES[self.shape] // 4)

    def with_labels(self, query_labels, tri_labels):
        return Batch(self.shape, self.records, self.first, query_labels, tri_labels)

    def firsts(self) -> np.ndarray:
        """`first` of every query, wherever the shape keeps it"""
        if self.shape == "contact":
            return np.zeros(self.n, np.int32) if self.first is None else np.asarray(self.first, np.int32)
        return self.rows()[:, 3].view(np.int32).copy()

    def statement(self, tris, grid=None) -> dict:
        if self.shape == "box":
            return scene.box_lists(tris, self.records, grid=grid)
        if self.shape == "contact":
            return scene.contact_lists(tris, self.records, first=self.first, query_labels=self.query_labels, tri_labels=self.tri_labels, grid=grid)
        return scene.obb_lists(tris, self.records, query_labels=self.query_labels, tri_labels=self.tri_labels, grid=grid)


def fixture_batch(shape: str, fixture, name: str, tris, labelled: bool = False) -> Batch:
    """the 4096 queries of a scene of the shape's fixture; labelled: with the labels the fixture's `*_lab_*` answers were made with"""
    if shape == "box":
        assert not labelled
        return Batch(shape, V.scene_boxes(fixture, name, tris))
    if shape == "contact":
        q, first, lab = W.scene_queries(fixture, name, tris)
        return Batch(shape, q, first, lab, W.scene_labels(name, tris.shape[0])) if labelled else Batch(shape, q, first)
    q, lab = OB.scene_queries(fixture, name, tris)
    return Batch(shape, q, None, lab, OB.scene_labels(tris.shape[0])) if labelled else Batch(shape, q)


def deep_batches(name, tris):
    """the queries of a deep scene: D.boxes (and for `nested` the boxes around its clusters as well), D.contact_queries, and the boxes as oriented boxes,
    rotated about their centres"""
    boxes = D.boxes(tris) if name != "nested" else np.concatenate([D.boxes(tris), D.make_boxes(name, tris)])
    c = ((boxes[:, 0:3] + boxes[:, 4:7]) * np.float32(0.5)).astype(np.float32); h = ((boxes[:, 4:7] - boxes[:, 0:3]) * np.float32(0.5)).astype(np.float32)
    obbs = OB._rotated(c, scene.make_rotations(D.SEED + 30, boxes.shape[0]), h)
    return [Batch("box", boxes), Batch("contact", D.contact_queries(name, tris)), Batch("obb", obbs)]


def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("overlap_lists_host", directory, sanitize)


def words(e) -> np.ndarray:
    return np.ascontiguousarray(e).view(np.uint64).reshape(-1)


def poisoned(capacity: int) -> np.ndarray:
    return np.full(int(capacity), POISON, dtype=np.uint64).view(ENTRY)


_EMPTY = np.zeros(0, dtype=np.int32)


def _batch_files(d, b: Batch):
    return [_host.put(d, "ol_records", b.rows()), _host.put(d, "ol_first", _EMPTY if b.first is None or b.shape != "contact" else np.asarray(b.first, np.int32)),
            _host.put(d, "ol_qlabels", _EMPTY if b.query_labels is None else np.asarray(b.query_labels, np.int32)),
            _host.put(d, "ol_tlabels", _EMPTY if b.tri_labels is None else np.asarray(b.tri_labels, np.int32))]


def host_brute(exe: str, directory, tris, b: Batch, grid=None) -> dict:
    """RefList under brute_force / tris_brute_force / obb_brute_force, then unique_segment: the lists in CSR form (offsets, ids).  grid: (min, max) of the grid
    box, None: scene.grid_box(tris)"""
    d = str(directory)
    glo, ghi = scene.grid_box(tris) if grid is None else grid
    par = os.path.join(d, "ol_brute_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<2i3f3f", SHAPE_CODE[b.shape], b.n, *[float(v) for v in glo], *[float(v) for v in ghi]))
    out_o, out_i = os.path.join(d, "ol_brute_offsets.bin"), os.path.join(d, "ol_brute_ids.bin")
    subprocess.run([exe, "brute", par, _host.put(d, "ol_tris", np.ascontiguousarray(tris, dtype=np.float32)), *_batch_files(d, b), out_o, out_i], check=True, timeout=1200)
    return {"offsets": np.fromfile(out_o, dtype=np.int64), "ids": np.fromfile(out_i, dtype=np.int32)}


def _walk(exe, d, grid, tris, b: Batch, offsets, entries):
    given = offsets is not None
    par = os.path.join(d, "ol_walk_params.bin")
    with open(par, "wb") as f:
        f.write(_host.grid_header(grid) + struct.pack("<iiiq", SHAPE_CODE[b.shape], b.n, 1 if given else 0, int(np.asarray(entries).shape[0]) if given else 0))
    f_off = _host.put(d, "ol_walk_offsets", np.ascontiguousarray(offsets, dtype=np.int64) if given else np.zeros(0, np.int64))
    f_ent = _host.put(d, "ol_walk_entries", np.ascontiguousarray(entries).view(ENTRY) if given else np.zeros(0, ENTRY))
    outs = [os.path.join(d, "ol_walk_" + x + ".bin") for x in ("counts", "totals", "list_offsets", "list_ids")]
    subprocess.run([exe, "walk", par, *_host.grid_files(d, grid, "ol_"), _host.put(d, "ol_tris", np.ascontiguousarray(tris, dtype=np.float32)), *_batch_files(d, b), f_off, f_ent, *outs],
                   check=True, timeout=1200)
    return f_off, f_ent, outs


def host_lists(exe: str, directory, grid: dict, tris, b: Batch) -> dict:
    """the whole protocol on the host over grid arrays: CSR lists and "refs" (R per query), "ref_offsets", "ref_entries" (the filled references before the
    sort), "totals" (the fill launch's six) and "counts" ((n, 4): R, cells visited, tests, blocks pruned)"""
    f_off, f_ent, outs = _walk(exe, str(directory), grid, tris, b, None, None)
    counts = np.fromfile(outs[0], dtype=np.int32).reshape(b.n, 4)
    return {"offsets": np.fromfile(outs[2], dtype=np.int64), "ids": np.fromfile(outs[3], dtype=np.int32), "refs": counts[:, 0].copy(), "ref_offsets": np.fromfile(f_off, dtype=np.int64),
            "ref_entries": np.fromfile(f_ent, dtype=ENTRY), "totals": np.fromfile(outs[1], dtype=np.int64), "counts": counts}


def host_fill(exe: str, directory, grid: dict, tris, b: Batch, offsets, entries):
    """fill mode into a copy of `entries` (capacity slots, the caller's poison) with the caller's offsets: (counts (n, 4), the six totals, the entries afterwards)"""
    _, f_ent, outs = _walk(exe, str(directory), grid, tris, b, offsets, entries)
    return np.fromfile(outs[0], dtype=np.int32).reshape(b.n, 4), np.fromfile(outs[1], dtype=np.int64), np.fromfile(f_ent, dtype=ENTRY)


def assert_csr_equal(got: dict, want: dict, what: str):
    go, wo = np.asarray(got["offsets"]), np.asarray(want["offsets"])
    assert go.shape == wo.shape, f"{what}: {go.shape} against {wo.shape} offsets"
    bad = np.flatnonzero(np.diff(go) != np.diff(wo))
    assert bad.size == 0, f"{what}: {bad.size} list lengths differ, first at {bad[:5]}: {np.diff(go)[bad[:5]]} against {np.diff(wo)[bad[:5]]}"
    bad = np.flatnonzero(np.asarray(got["ids"]) != np.asarray(want["ids"]))
    assert bad.size == 0, f"{what}: {bad.size} ids differ, the first in list {np.searchsorted(wo, bad[0], side='right') - 1}"


def csr_slice(csr: dict, which) -> dict:
    """the lists `which` of a CSR set, as a CSR set"""
    off = np.asarray(csr["offsets"])
    which = np.asarray(which)
    sizes = (off[which + 1] - off[which]).astype(np.int64)
    o = np.zeros(which.size + 1, np.int64); np.cumsum(sizes, out=o[1:])
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in which]) if which.size else np.zeros(0, np.int64)
    return {"offsets": o, "ids": np.asarray(csr["ids"])[idx.astype(np.int64)]}


def first_ids(csr: dict, k: int = 8) -> np.ndarray:
    """(n, k) int32: the first k ids of every list, unused slots -1 -- what the k-list reports"""
    off = np.asarray(csr["offsets"]); ids = np.asarray(csr["ids"])
    n = off.size - 1
    out = np.full((n, k), -1, dtype=np.int32)
    sizes = np.diff(off)
    for j in range(k):
        has = sizes > j
        out[has, j] = ids[off[:-1][has] + j]
    return out


def assert_fixture(csr: dict, fixture, key: str, what: str):
    """len(list i) == sizes[i], and the first min(8, len) ids == ids[i]"""
    sizes = np.diff(np.asarray(csr["offsets"]))
    bad = np.flatnonzero(sizes != fixture[key + "_sizes"])
    assert bad.size == 0, f"{what}: {bad.size} list lengths differ from the fixture's, first at {bad[:5]}"
    bad = np.flatnonzero((first_ids(csr) != fixture[key + "_ids"]).any(axis=1))
    assert bad.size == 0, f"{what}: the first ids of {bad.size} lists differ from the fixture's, first at {bad[:5]}"


# ---- the device ------------------------------------------------------------------------------------------------------------------

class DeviceBatch:
    """a Batch uploaded: device addresses of records, first and labels"""
    def __init__(self, mem, b: Batch, d_tri_labels=None):
        self.mem, self.b, self.n = mem, b, b.n
        self.d_records = mem.upload(b.rows())
        self.d_first = mem.upload(np.asarray(b.first, np.int32)) if (b.shape == "contact" and b.first is not None) else 0
        self.d_ql = mem.upload(np.ascontiguousarray(b.query_labels, dtype=np.int32)) if b.query_labels is not None else 0
        self.own_tl = b.tri_labels is not None and d_tri_labels is None
        self.d_tl = (mem.upload(np.ascontiguousarray(b.tri_labels, dtype=np.int32)) if self.own_tl else (d_tri_labels or 0)) if b.tri_labels is not None else 0

    def free(self):
        for p in (self.d_records, self.d_first, self.d_ql, self.d_tl if self.own_tl else 0):
            if p:
                self.mem.free(p)


def device_refs(api, grid, d_tris, db: DeviceBatch, n=None, skip: int = 0, **kw):
    """api.box_refs / tri_refs / obb_refs for the batch's shape; n, skip: a sub-batch of n queries starting at query `skip`"""
    b = db.b
    n = db.n if n is None else n
    rec = db.d_records + RECORD_BYTES[b.shape] * skip
    if b.shape == "box":
        return api.box_refs(grid, d_tris, rec, n, **kw)
    if b.shape == "contact":
        return api.tri_refs(grid, d_tris, rec, n, first=db.d_first + 4 * skip if db.d_first else 0, query_labels=db.d_ql + 12 * skip if db.d_ql else 0, tri_labels=db.d_tl, **kw)
    return api.obb_refs(grid, d_tris, rec, n, query_labels=db.d_ql + 4 * skip if db.d_ql else 0, tri_labels=db.d_tl, **kw)


def device_lists(c, grid, db: DeviceBatch, n=None, skip: int = 0):
    """the protocol on the device with poisoned, guarded buffers and numpy scans: CSR lists plus "refs", "ref_offsets", "ref_entries" (the filled references
    before the sort), "totals" (the fill launch's six), "unique_totals", "compact_totals"; every slot of every buffer must have been written"""
    import _poison as P
    api, mem = c.api, c.mem
    n = db.n if n is None else n
    d_counts = P.alloc_out(mem, 4 * n)
    device_refs(api, grid, c.d_tris, db, n, skip, counts=d_counts)
    mem.synchronize()
    refs = P.fetch(mem, d_counts, np.int32, n).copy()
    assert (refs >= 0).all()
    ro = np.zeros(n + 1, np.int64); np.cumsum(refs, out=ro[1:])
    total = int(ro[-1])
    d_ro = mem.upload(ro)
    d_e = P.alloc_out(mem, 8 * total)
    d_tot = mem.alloc(48); mem.zero(d_tot, 48)
    P.poison(mem, d_counts, 4 * n)
    device_refs(api, grid, c.d_tris, db, n, skip, counts=d_counts, offsets=d_ro, entries=d_e, capacity=total, counters=d_tot)
    mem.synchronize()
    assert (P.fetch(mem, d_counts, np.int32, n) == refs).all(), "fill mode counts what count mode counted"
    filled = P.fetch(mem, d_e, ENTRY, total).copy()
    P.assert_all_written(words(filled))
    totals = mem.download(d_tot, np.int64, 6).copy()
    P.poison(mem, d_counts, 4 * n)
    d_ut = mem.alloc(32); mem.zero(d_ut, 32)
    api.unique_lists(n, d_ro, d_e, total, d_counts, counters=d_ut, mem=mem)
    mem.synchronize()
    m = P.fetch(mem, d_counts, np.int32, n).copy()
    sorted_e = P.fetch(mem, d_e, ENTRY, total).copy()
    off = np.zeros(n + 1, np.int64); np.cumsum(m, out=off[1:])
    d_off = mem.upload(off)
    d_out = P.alloc_out(mem, 8 * int(off[-1]))
    d_ct = mem.alloc(32); mem.zero(d_ct, 32)
    api.compact_lists(n, d_ro, d_e, total, d_counts, d_off, d_out, int(off[-1]), counters=d_ct, mem=mem)
    mem.synchronize()
    out = P.fetch(mem, d_out, ENTRY, int(off[-1])).copy()
    P.assert_all_written(words(out))
    assert (out["d2"].view(np.uint32) == 0).all(), "the distance word of every entry is +0.0"
    res = {"offsets": off, "ids": out["id"].copy(), "refs": refs, "ref_offsets": ro, "ref_entries": filled, "sorted_entries": sorted_e,
           "totals": totals, "unique_totals": mem.download(d_ut, np.int64, 4).copy(), "compact_totals": mem.download(d_ct, np.int64, 4).copy()}
    for p in (d_counts, d_ro, d_e, d_tot, d_ut, d_off, d_out, d_ct):
        mem.free(p)
    return res
