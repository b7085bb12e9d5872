"""What the ball-list tests and the fixture generator (tests/golden/make_golden_ball_lists.py) share: the queries (those of _closest with finite radii), the host
program tests/cpp/ball_lists_host.cpp as callables (the brute-force lists, the walk with RefSink in count and fill mode, unique and compact over segments), the
synthetic segments of the second stage, the protocol on the device, and the fixture tests/golden/ball_lists.npz."""
import os
import struct
import subprocess

import numpy as np

from hagrid_amd import scene

import _closest as K
import _host
from _host import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "ball_lists.npz")
ENTRY = scene.NEAREST_ENTRY_DTYPE
SORT_CAP = 1024                                       # kSortCap of hagrid_amd/csrc/ball_lists.hip: what a wavefront sorts in LDS
# the queries whose full lists the fixture stores: RADIUS, SPECIAL and the first 64 NEAR ones
STORED = np.concatenate([np.arange(K.RADIUS.start, K.RADIUS.stop), np.arange(K.SPECIAL.start, K.SPECIAL.stop), np.arange(K.NEAR.start, K.NEAR.start + 64)])
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)                # an entry no launch wrote (tests/_poison.py): d2 a NaN, id -1


def queries(tris: np.ndarray) -> np.ndarray:
    """the 4096 queries of _closest with every r = +inf replaced by 5 % of the diagonal, and 50 % for the first eight UNIFORM ones (lists of thousands)"""
    q = K.fixture_queries(tris)
    lo, hi = scene.tris_bbox(tris)
    diag = K.diagonal(lo, hi)
    inf = np.isposinf(q[:, 3])
    q[inf, 3] = np.float32(0.05) * diag
    first = np.arange(K.UNIFORM.start, K.UNIFORM.start + 8)
    assert inf[first].all()
    q[first, 3] = np.float32(0.5) * diag
    return q


def build_host(directory, sanitize: bool = False) -> str:
    return _host.build_host("ball_lists_host", directory, sanitize)


def entries_of(d2, ids) -> np.ndarray:
    e = np.zeros(np.shape(ids), dtype=ENTRY)
    e["d2"] = d2; e["id"] = ids
    return e


def words(e) -> np.ndarray:
    return np.ascontiguousarray(e).view(np.uint64).reshape(-1)


def poisoned(capacity: int) -> np.ndarray:
    return np.full(int(capacity), POISON, dtype=np.uint64).view(ENTRY)


def _label_files(d, n, query_labels, tri_labels):
    empty = np.zeros(0, np.int32)
    return [_host.put(d, "bl_qlabels", empty if query_labels is None else np.ascontiguousarray(query_labels, dtype=np.int32)),
            _host.put(d, "bl_tlabels", empty if query_labels is None else np.ascontiguousarray(tri_labels, dtype=np.int32))]


def host_brute(exe: str, directory, tris, points, query_labels=None, tri_labels=None) -> dict:
    """brute_force of closest.h with RefSink, then unique_segment of unique_lists.h: the lists in CSR form (offsets, ids, d2) as scene.tris_within gives them"""
    d = str(directory); n = points.shape[0]
    par = os.path.join(d, "bl_brute_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<ii", n, 0 if query_labels is None else 1))
    out_o, out_e = os.path.join(d, "bl_brute_offsets.bin"), os.path.join(d, "bl_brute_entries.bin")
    subprocess.run([exe, "brute", par, _host.put(d, "bl_tris", np.ascontiguousarray(tris, dtype=np.float32)), _host.put(d, "bl_points", np.ascontiguousarray(points, dtype=np.float32)),
                    *_label_files(d, n, query_labels, tri_labels), out_o, out_e], check=True, timeout=1200)
    e = np.fromfile(out_e, dtype=ENTRY)
    return {"offsets": np.fromfile(out_o, dtype=np.int64), "ids": e["id"].copy(), "d2": e["d2"].copy()}


def host_refs(exe: str, directory, grid: dict, tris, points, offsets=None, entries=None, query_labels=None, tri_labels=None):
    """closest_query of closest.h with RefSink over grid arrays.  offsets None: count mode.  Else fill mode into a copy of `entries` (capacity slots, the
    caller's poison).  Returns (counts (n, 4) int32: R, cells visited, triangles tested, pruned; the six totals int64; the entries afterwards or None)"""
    d = str(directory); n = points.shape[0]
    fill = offsets is not None
    capacity = 0 if not fill else int(np.asarray(entries).shape[0])
    par = os.path.join(d, "bl_refs_params.bin")
    with open(par, "wb") as f:
        f.write(_host.grid_header(grid) + struct.pack("<iiiq", n, 0 if query_labels is None else 1, 1 if fill else 0, capacity))
    f_off = _host.put(d, "bl_refs_offsets", np.zeros(0, np.int64) if not fill else np.ascontiguousarray(offsets, dtype=np.int64))
    f_ent = _host.put(d, "bl_refs_entries", np.zeros(0, ENTRY) if not fill else np.ascontiguousarray(entries).view(ENTRY))
    out_c, out_t = os.path.join(d, "bl_refs_counts.bin"), os.path.join(d, "bl_refs_totals.bin")
    subprocess.run([exe, "refs", par, *_host.grid_files(d, grid, "bl_"), _host.put(d, "bl_tris", np.ascontiguousarray(tris, dtype=np.float32)),
                    _host.put(d, "bl_points", np.ascontiguousarray(points, dtype=np.float32)), *_label_files(d, n, query_labels, tri_labels), f_off, f_ent, out_c, out_t],
                   check=True, timeout=1200)
    return np.fromfile(out_c, dtype=np.int32).reshape(n, 4), np.fromfile(out_t, dtype=np.int64), (np.fromfile(f_ent, dtype=ENTRY) if fill else None)


def host_unique(exe: str, directory, offsets, entries):
    """unique_segment of unique_lists.h (the network the kernel runs) over every segment: (entries afterwards, counts int32)"""
    d = str(directory)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64); n = offsets.size - 1
    par = os.path.join(d, "bl_unique_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<iq", n, int(np.asarray(entries).shape[0])))
    f_ent = _host.put(d, "bl_unique_entries", np.ascontiguousarray(entries).view(ENTRY))
    out_c = os.path.join(d, "bl_unique_counts.bin")
    subprocess.run([exe, "unique", par, _host.put(d, "bl_unique_offsets", offsets), f_ent, out_c], check=True, timeout=1200)
    return np.fromfile(f_ent, dtype=ENTRY), np.fromfile(out_c, dtype=np.int32)


def host_compact(exe: str, directory, offsets, entries, counts, out_offsets, out_entries):
    """compact over every segment into a copy of out_entries (the caller's poison): the entries afterwards"""
    d = str(directory)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64); n = offsets.size - 1
    par = os.path.join(d, "bl_compact_params.bin")
    with open(par, "wb") as f:
        f.write(struct.pack("<iqq", n, int(np.asarray(entries).shape[0]), int(np.asarray(out_entries).shape[0])))
    f_out = _host.put(d, "bl_compact_out", np.ascontiguousarray(out_entries).view(ENTRY))
    subprocess.run([exe, "compact", par, _host.put(d, "bl_compact_offsets", offsets), _host.put(d, "bl_compact_entries", np.ascontiguousarray(entries).view(ENTRY)),
                    _host.put(d, "bl_compact_counts", np.ascontiguousarray(counts, dtype=np.int32)), _host.put(d, "bl_compact_out_offsets", np.ascontiguousarray(out_offsets, dtype=np.int64)),
                    f_out], check=True, timeout=1200)
    return np.fromfile(f_out, dtype=ENTRY)


def host_lists(exe: str, directory, grid: dict, tris, points, query_labels=None, tri_labels=None) -> dict:
    """the whole protocol on the host: count, scan, fill, unique, scan, compact.  CSR lists and "refs" (R per query), "ref_offsets", "ref_entries" (the filled
    references before the sort) and "totals" (the fill launch's six)"""
    counts, _, _ = host_refs(exe, directory, grid, tris, points, query_labels=query_labels, tri_labels=tri_labels)
    ro = np.zeros(points.shape[0] + 1, np.int64); np.cumsum(counts[:, 0], out=ro[1:])
    counts2, totals, filled = host_refs(exe, directory, grid, tris, points, offsets=ro, entries=poisoned(ro[-1]), query_labels=query_labels, tri_labels=tri_labels)
    assert (counts2 == counts).all()
    sorted_e, m = host_unique(exe, directory, ro, filled)
    off = np.zeros(points.shape[0] + 1, np.int64); np.cumsum(m, out=off[1:])
    out = host_compact(exe, directory, ro, sorted_e, m, off, poisoned(off[-1]))
    return {"offsets": off, "ids": out["id"].copy(), "d2": out["d2"].copy(), "refs": counts[:, 0].copy(), "ref_offsets": ro, "ref_entries": filled, "totals": totals,
            "counts": counts}


def assert_csr_equal(got: dict, want: dict, what: str):
    """offsets, ids, and the BITS of d2"""
    go, wo = np.asarray(got["offsets"]), np.asarray(want["offsets"])
    assert go.shape == wo.shape, f"{what}: {go.shape} against {wo.shape} offsets"
    bad = np.flatnonzero(np.diff(go) != np.diff(wo))
    assert bad.size == 0, f"{what}: {bad.size} list lengths differ, first at {bad[:5]}: {np.diff(go)[bad[:5]]} against {np.diff(wo)[bad[:5]]}"
    bad = np.flatnonzero((np.asarray(got["ids"]) != np.asarray(want["ids"])) | (K.bits(got["d2"]) != K.bits(want["d2"])))
    assert bad.size == 0, f"{what}: {bad.size} entries differ, the first in list {np.searchsorted(wo, bad[0], side='right') - 1}"


def csr_slice(csr: dict, which) -> dict:
    """the lists `which` of a CSR set, as a CSR set"""
    off = np.asarray(csr["offsets"])
    which = np.asarray(which)
    sizes = (off[which + 1] - off[which]).astype(np.int64)
    o = np.zeros(which.size + 1, np.int64); np.cumsum(sizes, out=o[1:])
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in which]) if which.size else np.zeros(0, np.int64)
    return {"offsets": o, "ids": np.asarray(csr["ids"])[idx], "d2": np.asarray(csr["d2"])[idx]}


# ---- synthetic segments for the second stage ---------------------------------------------------------------------------------------

SEGMENT_LENGTHS = (0, 1, 2, 63, 64, 65, SORT_CAP - 1, SORT_CAP, SORT_CAP + 1, 3 * SORT_CAP + 7, 20000)


def synthetic_segments(seed: int = 0x62616C6C):
    """(offsets int64 (n + 1,), entries (capacity,), capacity): three segments of every length of SEGMENT_LENGTHS in a shuffled order with gaps of poison between
    them, then segments whose range is refused (negative, decreasing, beyond the capacity: room 0).  A segment holds few distinct ids, each many times with
    ONE d2 per id (the contract), d2 drawn from few values so that ties in d2 between ids are common, +0.0 and -0.0 among them; about a sixth of its slots
    hold what must be dropped: the EMPTY entry, other negative ids, a NaN d2 -- in the middle, not at the end."""
    rng = np.random.RandomState(seed & 0x7fffffff)
    lengths = np.array(sorted(SEGMENT_LENGTHS * 3), dtype=np.int64)
    rng.shuffle(lengths)
    segs, offsets_b, offsets_e, pos = [], [], [], 5
    for L in lengths:
        L = int(L)
        distinct = max(1, min(L, int(rng.choice([1, 3, max(1, L // 7), max(1, L // 2), L]))))
        ids = rng.choice(1 << 20, size=distinct, replace=False).astype(np.int32)
        values = np.float32(rng.choice([0.0, -0.0, 0.25, 0.5, 1.0, 3.0, np.inf], size=8).tolist() + rng.rand(8).tolist())
        d2_of_id = values[rng.randint(0, values.size, size=distinct)]
        pick = rng.randint(0, distinct, size=L)
        if L >= distinct:
            pick[rng.permutation(L)[:distinct]] = np.arange(distinct)          # every id at least once
        e = entries_of(d2_of_id[pick], ids[pick])
        junk = rng.rand(L) < 1.0 / 6.0
        kind = rng.randint(0, 3, size=L)
        e["d2"][junk & (kind == 0)] = np.float32(np.inf); e["id"][junk & (kind == 0)] = -1
        e["id"][junk & (kind == 1)] = -7
        e["d2"][junk & (kind == 2)] = np.float32(np.nan)
        segs.append((pos, e))
        offsets_b.append(pos); offsets_e.append(pos + L)
        pos += L + int(rng.randint(0, 4))
    capacity = pos + 3
    entries = poisoned(capacity)
    for first, e in segs:
        entries[first:first + e.size] = e
    # CSR offsets need consecutive segments: segment i is [o[i], o[i + 1]) -- so the gaps are segments of their own, and the refused ranges are made by
    # offsets that step back or out
    o = [2]                                                       # slots 0 and 1, and the three behind the last segment, belong to nobody
    for b, e in zip(offsets_b, offsets_e):
        if o[-1] != b:
            o.append(b)
        o.append(e)
    if o[-1] != pos:
        o.append(pos)
    o += [capacity + 4, 7, -3, 2]                                 # beyond the capacity, decreasing, to a negative end, from a negative start: room 0 each
    return np.array(o, dtype=np.int64), entries, capacity


def tight_destination(counts, seed: int = 11):
    """(out_offsets, out_capacity) for compact over `counts`: most segments get exactly their count, some one slot less (too little room: a prefix is copied), some
    three slots more (padding), one a refused range"""
    rng = np.random.RandomState(seed)
    counts = np.asarray(counts, dtype=np.int64)
    room = counts.copy()
    how = rng.randint(0, 6, size=counts.size)
    room[(how == 0) & (counts > 0)] -= 1
    room[how == 1] += 3
    o = np.zeros(counts.size + 1, np.int64); np.cumsum(room, out=o[1:])
    capacity = int(o[-1])
    if counts.size > 4:
        capacity = int(o[-2])                                   # the last segment leaves the capacity: room 0
    return o, capacity


# ---- the device ------------------------------------------------------------------------------------------------------------------

def device_lists(c, grid, d_points, n, d_query_labels=0, d_tri_labels=0):
    """the protocol on the device with poisoned, guarded buffers and numpy scans: CSR lists plus "refs", "ref_offsets", "ref_entries" (the filled references
    before the sort), "totals" (the fill launch's six), "unique_totals", "compact_totals"; every slot of every buffer must have been written"""
    import _poison as P
    api, mem = c.api, c.mem
    d_counts = P.alloc_out(mem, 4 * n)
    api.ball_refs(grid, c.d_tris, d_points, n, counts=d_counts, query_labels=d_query_labels, tri_labels=d_tri_labels)
    mem.synchronize()
    refs = P.fetch(mem, d_counts, np.int32, n).copy()
    assert (refs >= 0).all()
    ro = np.zeros(n + 1, np.int64); np.cumsum(refs, out=ro[1:])
    total = int(ro[-1])
    d_ro = mem.upload(ro)
    d_e = P.alloc_out(mem, 8 * total)
    d_tot = mem.alloc(48); mem.zero(d_tot, 48)
    P.poison(mem, d_counts, 4 * n)
    api.ball_refs(grid, c.d_tris, d_points, n, counts=d_counts, offsets=d_ro, entries=d_e, capacity=total, query_labels=d_query_labels, tri_labels=d_tri_labels, counters=d_tot)
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
    res = {"offsets": off, "ids": out["id"].copy(), "d2": out["d2"].copy(), "refs": refs, "ref_offsets": ro, "ref_entries": filled, "sorted_entries": sorted_e,
           "totals": totals, "unique_totals": mem.download(d_ut, np.int64, 4).copy(), "compact_totals": mem.download(d_ct, np.int64, 4).copy()}
    for p in (d_counts, d_ro, d_e, d_tot, d_ut, d_off, d_out, d_ct):
        mem.free(p)
    return res


def fixture_csr(fixture, name: str) -> dict:
    """the stored lists of one scene (the queries STORED) as a CSR set"""
    sizes = fixture[name + "_sizes"][STORED].astype(np.int64)
    o = np.zeros(STORED.size + 1, np.int64); np.cumsum(sizes, out=o[1:])
    return {"offsets": o, "ids": fixture[name + "_ids"], "d2": fixture[name + "_d2"].view(np.float32)}
