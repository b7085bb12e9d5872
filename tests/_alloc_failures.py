"""What test_alloc_failures_cpu.py and test_alloc_failures_gpu.py share: the fixture scene, the table of allocation sites, what is expected of every entry point
when its i-th allocation request fails (include/hagrid_amd.h, "HAGRID_ENOMEM"), and the post-conditions as functions of plain values, so that the CPU test can
run them on hand-made states.

An allocation REQUEST is a call of hagrid_mem_alloc, a growth of the look-back status words or one of the context's own small device buffers
(hagrid_amd/csrc/ctx.hip: mem_request).  "mem.fail_request" = i of the test library makes the i-th request from now fail; "mem.fail_scan" = j makes the j-th look-back
scan from now find its status words gone and their growth refused (the exits behind a scan of a late level or iteration: the words of a pass only grow at its first
scan); hagrid_kat_mem_state reads the books."""
import glob
import os

import numpy as np

from hagrid_amd import scene

OK, EINVAL, EHIP, ENOMEM = 0, -1, -2, -3

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hagrid_amd", "csrc")

# ---- the allocation sites, counted by name ------------------------------------------------------------------------------------------------
# Every name under which a pass asks for device memory.  ".get<" is Temps / PoolTemps / Arena; "scan_plain(" and "ctx_scan<" reach lookback_state; "device_request("
# is the context's own buffers (status words, row scores, tile order, binning words).
SITE_NAMES = ("pool_alloc<", "pool_try_alloc<", ".get<", "hagrid_mem_alloc(", "lookback_state(", "ctx_scan<", "device_request(", "scan_plain(")

# file -> ({name: occurrences in the file}, the entry points of the sweep that reach them).  A site added later changes a count: it has to be entered here, with the
# entry point whose sweep then covers it.  (ctx.hip: the three pool_alloc of hagrid_bandwidth_probe -- a diagnostic outside the sweep --, the definitions of
# hagrid_mem_alloc and lookback_state, device_request's definition and its use for the status words.  build.hip's scan_plain( is its definition.)
SITES = {
    "assemble.hip": ({"hagrid_mem_alloc(": 1}, ("scene_create",)),
    "blob.hip": ({".get<": 2, "hagrid_mem_alloc(": 3}, ("grid_pack", "grid_save", "grid_load")),          # (.get<, one hagrid_mem_alloc: hagrid_grid_broadcast, needs RCCL ranks)
    "build.hip": ({"pool_alloc<": 3, "pool_try_alloc<": 1, ".get<": 18, "ctx_scan<": 6, "scan_plain(": 1}, ("build_grid",)),
    "compress.hip": ({"pool_alloc<": 2, "hagrid_mem_alloc(": 1}, ("compress_grid",)),
    "ctx.hip": ({"pool_alloc<": 3, "hagrid_mem_alloc(": 1, "lookback_state(": 1, "device_request(": 2}, ()),
    "distance.hip": ({".get<": 1, "scan_plain(": 1}, ("distance_lattice",)),
    "expand.hip": ({"pool_alloc<": 2, "pool_try_alloc<": 2}, ("expand_grid",)),
    "flatten.hip": ({"pool_alloc<": 1, ".get<": 4, "ctx_scan<": 1}, ("flatten_grid",)),
    "merge.hip": ({"pool_alloc<": 9, "ctx_scan<": 3}, ("merge_grid",)),
    # (.get< and ctx_scan<: the binning buffers and their scan, both modes; device_request(: bin_diff -- automatic binning --, row_scores -- automatic binning and
    # the row detection, from 2^18 rays on --, lpt_buf -- un-binned launches that know their rows)
    "ray_order.hip": ({".get<": 4, "ctx_scan<": 2, "device_request(": 3}, ("traverse_grid_binned", "traverse_grid_auto_binned", "traverse_grid_tile_order", "traverse_grid_row_detect")),
    "trav_image.hip": ({"pool_alloc<": 9, "hagrid_mem_alloc(": 4, "ctx_scan<": 1}, ("setup_traversal",)),
    "traverse.hip": ({"pool_alloc<": 1}, ("traverse_grid_stats",)),
}


def count_sites(text: str) -> dict:
    """{name: occurrences} of the allocation names in a source text, names that do not occur left out"""
    c = {n: text.count(n) for n in SITE_NAMES}
    return {n: v for n, v in c.items() if v}


def source_site_counts(csrc: str = CSRC) -> dict:
    """{file: count_sites(file)} over hagrid_amd/csrc/*.hip (not kat/), files without a site left out"""
    out = {}
    for f in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        c = count_sites(open(f, encoding="utf-8").read())
        if c:
            out[os.path.basename(f)] = c
    return out


# ---- the entry points of the sweep ---------------------------------------------------------------------------------------------------------
# min_requests: the UNCONDITIONAL requests of the entry point, read from its source -- the measured number R must be at least that, so a counter that counts
#               nothing fails the sweep instead of emptying it.
# state:        what the header promises after HAGRID_ENOMEM: "unchanged" (descriptor and arrays byte for byte what they were), "released" (merge_grid: cells and
#               ref_ids back in the pool and NULL, entries still the caller's), "no_output" (an output handle / pointer that stays NULL or as it was).
# untouched:    compared output buffers keep every byte 0xFF after HAGRID_ENOMEM (no ENOMEM exit of these entry points lies behind the kernel that writes them;
#               where an exit lies behind OTHER launches -- binning, the size pass of the distance lattice -- those write temporaries and the workspace only).
# optional:     the requests whose failure is NOT an error -- optional_indices() below turns the rule into a set of indices.
ENTRY_POINTS = {
    "build_grid": dict(min_requests=4, state="unchanged", untouched=False, optional="arena"),                 # bb_part, out_cells, out_entries, out_refs (the rest: arena or pool)
    "merge_grid": dict(min_requests=9, state="released", untouched=False, optional=None),                     # the nine pool buffers in front of the loop
    "flatten_grid": dict(min_requests=5, state="unchanged", untouched=False, optional=None),                  # depths, start, collapsed, partials, out
    "expand_grid": dict(min_requests=2, state="unchanged", untouched=False, optional="expand"),               # other, flags
    "compress_grid": dict(min_requests=3, state="unchanged", untouched=False, optional=None),                 # partials, small, srefs
    "setup_traversal": dict(min_requests=5, state="unchanged", untouched=False, optional="second_table"),     # blocks: metas, offs, partials, table, recs; general: recs, 2 x items, claim, wide
    "traverse_grid_binned": dict(min_requests=4, state="unchanged", untouched=True, optional=None),           # perm, keys, table, partials
    "traverse_grid_auto_binned": dict(min_requests=5, state="unchanged", untouched=True, optional="row_scores"),  # perm, keys, table, partials, bin_diff (2^18 rays: + row_scores)
    "traverse_grid_tile_order": dict(min_requests=1, state="unchanged", untouched=True, optional="all"),      # the tile-order buffer (image width given, 8192 rays)
    "traverse_grid_row_detect": dict(min_requests=1, state="unchanged", untouched=True, optional="all"),      # row_scores (image width looked for, 2^18 rays; + the tile-order buffer)
    "traverse_grid_stats": dict(min_requests=1, state="unchanged", untouched=True, optional=None),            # the eight counters
    "distance_lattice": dict(min_requests=1, state="unchanged", untouched=True, optional=None),               # the task sizes
    "scene_create": dict(min_requests=1, state="no_output", untouched=False, optional=None),                  # the tables (hagrid_scene_assemble itself: none)
    "grid_pack": dict(min_requests=1, state="no_output", untouched=False, optional=None),
    "grid_save": dict(min_requests=1, state="no_output", untouched=False, optional=None),
    "grid_load": dict(min_requests=1, state="no_output", untouched=False, optional=None),
}
NO_REQUESTS = ("grid_unpack", "scene_assemble")             # outside the sweep: asserted to make no request

# The optional sites, read from the code (DESIGN.md section 6 has the same table with the indices the sweeps reported):
#   expand.hip  `list`         iters > 1: the third request         -> the list of cells is not taken
#   expand.hip  `voxel_cells`  the request behind it                -> the voxel map is not taken
#   build.hip   Arena          the second request of a context's second and later constructions (behind bb_part) -> the arena is not taken
#   trav_image.hip build_blocks, the compact layout next to a much bigger uniform one: its table, its records, its claim words and, with wide records, the buffer
#               of table + wide records -- requests 6 to 8 or 9 of the call, behind the five of the uniform layout -> the second table is not built
#   ray_order.hip row_scores, lpt_buf: every request of an un-binned launch -> the launch keeps its first criterion / its default order; row_scores also as the sixth
#               request of an automatically binned launch of 2^18 rays and more (bin_diff, the fifth, is a hard failure)
# hagrid_setup_traversal does NOT end without an image for lack of memory: every other request of it is a hard failure.


def optional_indices(entry: str, R: int, **cfg) -> list:
    """The set of indices 1 .. R that may come back OK, as a list of admissible sets (empty: R itself contradicts the source)."""
    rule = ENTRY_POINTS[entry]["optional"]
    if rule is None:
        return [set()]
    if rule == "arena":
        return [{2} if cfg.get("later_build") else set()]
    if rule == "expand":
        return [{3, 4} if cfg.get("iters", 1) > 1 else {3}]
    if rule == "second_table":
        if not cfg.get("two_layouts"):
            return [set()]
        return [set(range(6, R + 1))] if R in (8, 9) else []         # (in front of them: metas, offs, partials, table, the uniform layout's records)
    if rule == "row_scores":
        return [{6}] if R >= 6 else []                       # (behind perm, keys, table, partials and bin_diff)
    if rule == "all":
        return [set(range(1, R + 1))]
    raise KeyError(rule)


# ---- the fixture scene -----------------------------------------------------------------------------------------------------------------------

TOP_DENSITY, SND_DENSITY, ALPHA = 0.12, 2.4, 0.9999
EXPAND_ITERS = 3


def fixture_scene(n: int = 3000, seed: int = 31) -> np.ndarray:
    """make_soup(n) with half its triangles shrunk into a 3 % box (test_random_scenes_and_parameters, kind 2) inside the six wall quads of
    test_build_scene_with_huge_triangles: deep levels in the cluster, primitives on the cooperative list, a merge that runs long"""
    tris = scene.make_soup(n, seed=seed).copy()
    m = n // 2
    tris[:m, 0:3] = tris[:m, 0:3] * np.float32(0.03) + np.float32(0.6); tris[:m, 4:7] *= np.float32(0.03); tris[:m, 8:11] *= np.float32(0.03)
    e1, e2 = tris[:, 4:7], tris[:, 8:11]
    nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(np.float32)
    tris[:, 3] = nrm[:, 0]; tris[:, 7] = nrm[:, 1]; tris[:, 11] = nrm[:, 2]
    lo, hi = np.float32([-2, -0.05, -2]), np.float32([3, 1.5, 3])

    def quad(a, b, c, d):
        a, b, c, d = (np.float32(v)[None, :] for v in (a, b, c, d))
        return np.concatenate([scene.tris_from_vertices(a, b, c), scene.tris_from_vertices(a, c, d)])
    walls = [quad([lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], lo[1], hi[2]], [lo[0], lo[1], hi[2]]),
             quad([lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], lo[2]]),
             quad([lo[0], lo[1], hi[2]], [hi[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]),
             quad([lo[0], lo[1], lo[2]], [lo[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]], [lo[0], hi[1], lo[2]]),
             quad([hi[0], lo[1], lo[2]], [hi[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]], [hi[0], hi[1], lo[2]]),
             quad([lo[0], 0.4, lo[2]], [hi[0], 0.9, lo[2]], [hi[0], 0.2, hi[2]], [lo[0], 0.7, hi[2]])]
    return np.ascontiguousarray(np.concatenate([tris] + walls), dtype=np.float32)


def entered_in_place(merge_cells, merged_cells: int, alpha: float, div: int = 2) -> bool:
    """whether merge_grid entered its in-place mode, from the build counts alone: the cells that entered every axis pass (three per iteration) and the final count.
    merge.hip enters the mode behind a compacting iteration that merged less than 1 / div of its cells while the loop goes on (out < alpha * in)."""
    ins = [int(c) for c in merge_cells[0::3]] + [int(merged_cells)]
    for a, b in zip(ins[:-2], ins[1:-1]):                    # (an iteration whose successor exists: the loop went on)
        if div * (a - b) < a and b < alpha * a:
            return True
    return False


# ---- post-conditions on plain values ---------------------------------------------------------------------------------------------------------

BOOK_KEYS = ("slots_in_use", "tracked", "bytes_in_use")


def check_fired(pending_request: int):
    assert pending_request == 0, f"mem.fail_request reads back {pending_request}: the injected request was never made"


def check_error_text(rc: int, text: str, earlier: str):
    """after an injected failure: HAGRID_ENOMEM, a message, and not the message of the earlier (provoked) error"""
    assert rc == ENOMEM, f"return {rc}, not HAGRID_ENOMEM"
    assert text, "HAGRID_ENOMEM with an empty hagrid_last_error"
    assert text != earlier, f"hagrid_last_error still holds the earlier error: {text!r}"
    assert "hipMalloc failed" in text or "no host memory" in text, f"hagrid_last_error does not name the failure: {text!r}"


def check_books(before: dict, after: dict, released_slots: int = 0, released_bytes: int = 0, what: str = ""):
    """slots in use, tracked pointers and bytes in use after a call against their values before it, less what the call is documented to release
    (released_bytes = None: the released slots' sizes are not known to the caller)"""
    want = {"slots_in_use": before["slots_in_use"] - released_slots, "tracked": before["tracked"] - released_slots, "bytes_in_use": before["bytes_in_use"] - (released_bytes or 0)}
    got = {k: after[k] for k in BOOK_KEYS}
    if released_bytes is None:                              # how large the released slots were is the pool's choice: fewer bytes in use, the counts exact
        assert after["bytes_in_use"] < before["bytes_in_use"] or not released_slots, f"{what}: {released_slots} slots released and no byte less in use"
        want["bytes_in_use"] = got["bytes_in_use"]
    assert got == want, f"{what}: the pool's books are {got}, expected {want} (a buffer of the call stayed in use, or one was freed twice)"


def check_usage(before: int, after: int, what: str = ""):
    assert after == before, f"{what}: usage {after} after the call, {before} before it"


def check_outcomes(entry: str, R: int, ok_indices, admissible, what: str = ""):
    """the indices that came back OK are exactly a set the table admits; every other index is a hard failure"""
    assert R >= ENTRY_POINTS[entry]["min_requests"], f"{entry} {what}: {R} requests counted, the source has at least {ENTRY_POINTS[entry]['min_requests']} unconditional ones"
    got = set(ok_indices)
    assert any(got == set(a) for a in admissible), (f"{entry} {what}: requests {sorted(got)} of {R} degraded instead of failing, the table of optional sites predicts "
                                                    f"{' or '.join(str(sorted(a)) for a in admissible)}")


def check_untouched(raw, what: str = ""):
    """every byte still 0xFF (tests/_poison.py): the failed call wrote nothing into a compared output"""
    a = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    bad = np.flatnonzero(a != 0xFF)
    assert bad.size == 0, f"{what}: {bad.size} bytes of a compared output written by a call that failed, the first at byte {bad[0]}"


def check_descriptor_unchanged(before: bytes, after: bytes, what: str = ""):
    assert after == before, f"{what}: the descriptor changed in a call that failed"


def check_released(cells: int, ref_ids: int, num_cells: int, num_refs: int, entries: int, what: str = ""):
    """merge_grid after a failure: cells and ref_ids NULL with their counts, entries still named"""
    assert not cells and not ref_ids and num_cells == 0 and num_refs == 0, f"{what}: cells {cells:#x} / ref_ids {ref_ids:#x} ({num_cells}, {num_refs}) left in the descriptor of a grid that is gone"
    assert entries, f"{what}: entries are the caller's to free, the descriptor lost them"
