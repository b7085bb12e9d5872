"""What the neighbour-query tests and the fixture generator (tests/golden/make_golden_nearest_k.py) share: the host program tests/cpp/nearest_k_host.cpp
as callables (the brute-force definition and the walk over grid arrays, with cursors and labels), paging with any single-page function, and the fixture
tests/golden/nearest_k.npz.  Scenes and queries are those of _closest."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _closest as K
import _host
from _host import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "nearest_k.npz")
ENTRY = scene.NEAREST_ENTRY_DTYPE
KMAX = 8
PAGE_K, PAGES = 3, 3                                  # the fixture's paged part: the first three pages at k = 3
# the queries that are paged to their end: the ones with a radius, and the r = 0 queries on vertices and elsewhere
PAGED = np.concatenate([np.arange(K.RADIUS.start, K.RADIUS.stop), np.arange(K.SPECIAL.start + 32, K.SPECIAL.start + 48)])
# the queries whose first three pages the fixture stores
STORED = np.concatenate([np.arange(s.start, s.stop) for s in (K.RADIUS, K.VERTEX, K.SPECIAL)])


def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("nearest_k_host", directory, sanitize)


def entries_of(d2, ids) -> np.ndarray:
    e = np.zeros(np.shape(ids), dtype=ENTRY)
    e["d2"] = d2; e["id"] = ids
    return e


def _batch_files(d, prefix, n, k, tris, queries, cursors, query_labels, tri_labels, extra=b""):
    flags = struct.pack("<iiii", n, k, 0 if cursors is None else 1, 0 if query_labels is None else 1) + extra
    empty = np.zeros(0, np.int32)
    files = [_host.put(d, prefix + "tris", np.ascontiguousarray(tris, dtype=np.float32)), _host.put(d, prefix + "queries", np.ascontiguousarray(queries, dtype=np.float32)),
             _host.put(d, prefix + "cursors", empty if cursors is None else np.ascontiguousarray(cursors).view(ENTRY)),
             _host.put(d, prefix + "qlabels", empty if query_labels is None else np.ascontiguousarray(query_labels, dtype=np.int32)),
             _host.put(d, prefix + "tlabels", empty if query_labels is None else np.ascontiguousarray(tri_labels, dtype=np.int32))]
    return flags, files


def host_brute(exe: str, directory, tris, points, k: int, cursors=None, query_labels=None, tri_labels=None, prefix="nk_", record=scene.CLOSEST_DTYPE, extra=b""):
    """brute_force of include/hagrid/closest.h with the k-list: (entries (n, k), records (n, k)).  prefix, record, extra: the file names, the record and the
    parameters behind the flags of another list program (_segments)"""
    d = str(directory); n = points.shape[0]
    flags, files = _batch_files(d, prefix, n, k, tris, points, cursors, query_labels, tri_labels, extra)
    par = os.path.join(d, prefix + "brute_params.bin")
    with open(par, "wb") as f:
        f.write(flags)
    out_e, out_r = os.path.join(d, prefix + "brute_entries.bin"), os.path.join(d, prefix + "brute_records.bin")
    subprocess.run([exe, "brute", par, *files, out_e, out_r], check=True, timeout=1200)
    return np.fromfile(out_e, dtype=ENTRY).reshape(n, k), np.fromfile(out_r, dtype=record).reshape(n, k)


def host_walk(exe: str, directory, grid: dict, tris, points, k: int, cursors=None, query_labels=None, tri_labels=None, prefix="nk_", record=scene.CLOSEST_DTYPE, extra=b""):
    """closest_query of include/hagrid/closest.h with the k-list over grid arrays (what api.Grid.download returns): (entries (n, k), records (n, k), per-query
    counts (n, 4) int32: cells visited, triangles tested, pruned, list full)"""
    d = str(directory); n = points.shape[0]
    flags, files = _batch_files(d, prefix, n, k, tris, points, cursors, query_labels, tri_labels, extra)
    par = os.path.join(d, prefix + "walk_params.bin")
    with open(par, "wb") as f:
        f.write(_host.grid_header(grid) + flags)
    out_e, out_r, out_c = (os.path.join(d, prefix + "walk_" + x + ".bin") for x in ("entries", "records", "counts"))
    subprocess.run([exe, "walk", par, *_host.grid_files(d, grid, prefix), *files, out_e, out_r, out_c], check=True, timeout=1200)
    return (np.fromfile(out_e, dtype=ENTRY).reshape(n, k), np.fromfile(out_r, dtype=record).reshape(n, k), np.fromfile(out_c, dtype=np.int32).reshape(n, 4))


def run_lists(launch, record, mem, grid, d_tris, d_queries, n, k, cursors=None, query_labels=None, d_query_labels=0, d_tri_labels=0, counters=False, entries=True,
              records=True):
    """the lists of n queries on the device through launch (api.nearest_tris, api.segment_tris): (entries (n, k), records (n, k)[, the five counters]); outputs
    are poisoned, every slot must be written, the guard behind them must stay untouched; cursors and query labels (unless given as a device address) are
    uploaded"""
    import _poison as P
    d_e = P.alloc_out(mem, 8 * n * k) if entries else 0
    d_r = P.alloc_out(mem, 32 * n * k) if records else 0
    d_cur = mem.upload(np.ascontiguousarray(cursors)) if cursors is not None else 0
    d_ql = mem.upload(np.ascontiguousarray(query_labels, dtype=np.int32)) if query_labels is not None else 0
    d_cnt = 0
    if counters:
        d_cnt = mem.alloc(40); mem.zero(d_cnt, 40)
    ql = d_ql or d_query_labels
    launch(grid, d_tris, d_queries, n, k, entries=d_e, records=d_r, cursors=d_cur, query_labels=ql, tri_labels=d_tri_labels if ql else 0, counters=d_cnt)
    mem.synchronize()
    e = r = None
    if entries:
        e = P.fetch(mem, d_e, ENTRY, n * k).reshape(n, k).copy(); mem.free(d_e)
        P.assert_all_written(e.reshape(-1).view(np.uint64))
    if records:
        r = P.fetch(mem, d_r, record, n * k).reshape(n, k).copy(); mem.free(d_r)
        P.assert_all_written(r.reshape(-1))
    for p in (d_cur, d_ql):
        if p:
            mem.free(p)
    if counters:
        cnt = mem.download(d_cnt, np.int64, 5); mem.free(d_cnt)
        return e, r, cnt
    return e, r


def words(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape + (a.dtype.itemsize // 4,))


def assert_lists_equal(got, want, what: str):
    """entries or records, (n, k): every word equal, no query excepted"""
    g, w = words(got), words(want)
    assert g.shape == w.shape, f"{what}: {g.shape} against {w.shape}"
    bad = (g != w).reshape(g.shape[0], -1).any(axis=1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} queries differ, first at {np.flatnonzero(bad)[:5]}: got {got[bad][:1]}, want {want[bad][:1]}"


def page_through(ask, n: int, k: int, max_pages: int = 64):
    """Pages every query to its end the way a caller does.  ask(which, cursors) -> entries (len(which), k) for the queries `which` (cursors None on the
    first page).  The cursor of the next page is the last slot of a full list; a list that is not full is the last page.  Returns (lists: per query the
    concatenated (d2, id) entries, pages: per query how many pages were asked for)."""
    lists = [[] for _ in range(n)]
    pages = np.zeros(n, dtype=np.int64)
    which, cursors = np.arange(n), None
    for _ in range(max_pages):
        if which.size == 0:
            break
        e = ask(which, cursors)
        pages[which] += 1
        for row, i in zip(e, which):
            lists[i].append(row[row["id"] >= 0])
        full = e["id"][:, k - 1] >= 0
        which, cursors = which[full], np.ascontiguousarray(e[full][:, k - 1])
    assert which.size == 0, "paging did not end"
    return [np.concatenate(x) if x else np.zeros(0, ENTRY) for x in lists], pages


def first_pages(ask, n: int) -> np.ndarray:
    """(PAGES, n, PAGE_K) entries: the first PAGES pages of n queries at k = PAGE_K, every page asked of ALL queries.  ask(cursors) -> entries (n, PAGE_K);
    cursors: None on the first page, then (n,) entries: the last slot of the query's last FULL page, (-1, -1) while it has had none -- a query whose
    list was not full keeps its cursor and answers the same again."""
    out, cursors = [], None
    for _ in range(PAGES):
        e = ask(cursors)
        out.append(e)
        full = e["id"][:, -1] >= 0
        nxt = entries_of(np.full(n, -1.0, np.float32), np.full(n, -1, np.int32)) if cursors is None else cursors.copy()
        nxt[full] = e[full][:, -1]
        cursors = nxt
    return np.stack(out)


def assert_pages_equal_csr(lists, csr: dict, what: str):
    """the concatenated pages against scene.tris_within / api.tris_within (offsets, ids, d2): every id once, the same order, the same bits"""
    off = csr["offsets"]
    assert len(lists) == off.size - 1
    for i, l in enumerate(lists):
        s = slice(off[i], off[i + 1])
        assert l.size == off[i + 1] - off[i] and (l["id"] == csr["ids"][s]).all() and (K.bits(l["d2"]) == K.bits(csr["d2"][s])).all(), f"{what}: query {i}"


def fixture_lists(fixture, name: str):
    """(entries (4096, 8) of one scene of the fixture, its pages (PAGES, len(STORED), PAGE_K))"""
    e = entries_of(fixture[name + "_d2"].view(np.float32), fixture[name + "_id"])
    p = entries_of(fixture[name + "_page_d2"].view(np.float32), fixture[name + "_page_id"])
    return e, p


def stadium_labels():
    """the label case: the stadium mesh at 0.05, its vertices as queries (r = 2 % of the diagonal), label = vertex index, triangle labels = index triples"""
    V, F = scene.make_stadium_mesh(0.05)
    V = np.ascontiguousarray(V, np.float32); F = np.ascontiguousarray(F, np.int32)
    tris = scene.tris_from_mesh(V, F)
    lo, hi = scene.tris_bbox(tris)
    q = np.empty((V.shape[0], 4), dtype=np.float32)
    q[:, 0:3] = V; q[:, 3] = np.float32(0.02) * scene.bbox_diagonal(lo, hi)
    return tris, F, q, np.arange(V.shape[0], dtype=np.int32)
