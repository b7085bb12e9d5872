"""The table of allocation sites (tests/_alloc_failures.py) against the sources, the table's own consistency, and the post-conditions of the GPU sweep on hand-made
states -- without a GPU.  An allocation site added to a pass changes a count here: it has to be entered in the table, with the entry point whose sweep covers it."""
import os

import numpy as np
import pytest

import _alloc_failures as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_allocation_site_of_the_sources_is_in_the_table():
    found = A.source_site_counts()
    want = {f: c for f, (c, _) in A.SITES.items()}
    assert sorted(found) == sorted(want), f"files with allocation sites {sorted(found)}, the table lists {sorted(want)}"
    for f in sorted(found):
        assert found[f] == want[f], f"{f}: allocation sites {found[f]}, the table says {want[f]} -- enter the new site, and the entry point that reaches it"


def test_no_device_allocation_outside_the_one_helper():
    """hipMalloc for device buffers has one home (ctx.hip device_malloc) and one more use: the scratch words of hagrid_ctx_create, before there is a pool"""
    hits = {}
    for dirpath, _, files in os.walk(A.CSRC):
        for name in files:
            if name.endswith((".hip", ".h")):
                n = open(os.path.join(dirpath, name), encoding="utf-8").read().count("hipMalloc(")
                if n:
                    hits[os.path.relpath(os.path.join(dirpath, name), A.CSRC)] = n
    assert hits == {"ctx.hip": 2}, hits


def test_count_sites_counts_by_name():
    text = "int* a = pool_alloc<int>(ctx, n); auto b = tmp.get<float>(3); x = ar.get<int>(1);\nif (!ctx_scan<int>(ctx, In{}, Out{}, n)) return;  // pool_try_alloc<char>\n"
    assert A.count_sites(text) == {"pool_alloc<": 1, "pool_try_alloc<": 1, ".get<": 2, "ctx_scan<": 1}
    assert A.count_sites("hipMemcpyAsync(dst, src, n);") == {}


def test_the_table_is_consistent():
    swept = set(A.ENTRY_POINTS)
    reached = {e for _, entries in A.SITES.values() for e in entries}
    assert reached == swept, f"entry points of the sweep without a source file, or files without a swept entry point: {sorted(reached ^ swept)}"
    assert not set(A.NO_REQUESTS) & swept
    for name, spec in A.ENTRY_POINTS.items():
        assert spec["min_requests"] >= 1 and spec["state"] in ("unchanged", "released", "no_output"), name
        assert spec["optional"] in (None, "arena", "expand", "second_table", "row_scores", "all"), name
    # the unconditional requests are sites of the table: an entry point cannot promise more of them than its files hold
    per_entry = {}
    for counts, entries in A.SITES.values():
        for e in entries:
            per_entry[e] = per_entry.get(e, 0) + sum(counts.values())
    for name, spec in A.ENTRY_POINTS.items():
        assert spec["min_requests"] <= per_entry[name], name
    assert A.ENTRY_POINTS["merge_grid"]["min_requests"] == 9 and A.ENTRY_POINTS["expand_grid"]["min_requests"] == 2
    # the header states the contract of every entry point of the table
    header = open(os.path.join(ROOT, "include", "hagrid_amd.h"), encoding="utf-8").read()
    for fn in ("hagrid_build_grid", "hagrid_merge_grid", "hagrid_flatten_grid", "hagrid_expand_grid", "hagrid_compress_grid", "hagrid_setup_traversal", "hagrid_traverse_grid",
               "hagrid_traverse_grid_stats", "hagrid_distance_lattice", "hagrid_scene_create", "hagrid_grid_pack", "hagrid_grid_unpack", "hagrid_grid_save"):
        decl = header.index(f"int {fn}(")
        comment = header[header.rindex("/*", 0, decl):decl]
        assert "HAGRID_ENOMEM" in comment, f"{fn}: the comment in front of its declaration does not say what HAGRID_ENOMEM leaves behind"


def test_optional_indices():
    assert A.optional_indices("merge_grid", 12) == [set()]
    assert A.optional_indices("build_grid", 40) == [set()] and A.optional_indices("build_grid", 6, later_build=True) == [{2}]
    assert A.optional_indices("expand_grid", 3, iters=1) == [{3}] and A.optional_indices("expand_grid", 4, iters=3) == [{3, 4}]
    assert A.optional_indices("setup_traversal", 5) == [set()]
    assert A.optional_indices("setup_traversal", 8, two_layouts=True) == [{6, 7, 8}] and A.optional_indices("setup_traversal", 9, two_layouts=True) == [{6, 7, 8, 9}]
    assert A.optional_indices("setup_traversal", 7, two_layouts=True) == []
    assert A.optional_indices("traverse_grid_tile_order", 2) == [{1, 2}] and A.optional_indices("traverse_grid_row_detect", 1) == [{1}]
    assert A.optional_indices("traverse_grid_auto_binned", 6) == [{6}] and A.optional_indices("traverse_grid_auto_binned", 5) == []


def test_check_outcomes_on_hand_made_sweeps():
    A.check_outcomes("expand_grid", 4, [3, 4], A.optional_indices("expand_grid", 4, iters=3))
    A.check_outcomes("merge_grid", 11, [], A.optional_indices("merge_grid", 11))
    with pytest.raises(AssertionError, match="degraded instead of failing"):          # a hard failure that was swallowed
        A.check_outcomes("merge_grid", 11, [10], A.optional_indices("merge_grid", 11))
    with pytest.raises(AssertionError, match="degraded instead of failing"):          # an optional buffer that became mandatory
        A.check_outcomes("expand_grid", 4, [4], A.optional_indices("expand_grid", 4, iters=3))
    with pytest.raises(AssertionError, match="unconditional"):                        # a counter that counts nothing: not an empty sweep that passes
        A.check_outcomes("merge_grid", 0, [], A.optional_indices("merge_grid", 0))
    with pytest.raises(AssertionError, match="unconditional"):
        A.check_outcomes("expand_grid", 1, [], [set()])


def test_check_books_and_usage_on_hand_made_states():
    before = {"requests": 10, "mallocs": 4, "slots_in_use": 5, "tracked": 5, "bytes_in_use": 4096, "bytes_cached": 512}
    A.check_books(before, dict(before, requests=14, mallocs=6, bytes_cached=0))                 # the counters and the cache may move
    with pytest.raises(AssertionError, match="stayed in use"):
        A.check_books(before, dict(before, slots_in_use=6, tracked=6, bytes_in_use=4352))        # a slot in use for ever
    with pytest.raises(AssertionError, match="stayed in use"):
        A.check_books(before, dict(before, tracked=4))                                           # a pointer freed that the descriptor still names
    A.check_books(before, dict(before, slots_in_use=3, tracked=3, bytes_in_use=2048), released_slots=2, released_bytes=2048)
    A.check_books(before, dict(before, slots_in_use=3, tracked=3, bytes_in_use=1024), released_slots=2, released_bytes=None)
    with pytest.raises(AssertionError):
        A.check_books(before, dict(before, slots_in_use=3, tracked=3), released_slots=2, released_bytes=None)       # two slots gone, no byte less
    with pytest.raises(AssertionError):
        A.check_books(before, before, released_slots=2, released_bytes=2048)
    A.check_usage(1 << 20, 1 << 20)
    with pytest.raises(AssertionError, match="usage"):
        A.check_usage(1 << 20, (1 << 20) + 256)


def test_check_error_text_and_fired():
    earlier = "build.hip(989): build_grid: no triangles"
    A.check_error_text(A.ENOMEM, "ctx.hip(150): hipMalloc failed", earlier)
    with pytest.raises(AssertionError, match="not HAGRID_ENOMEM"):
        A.check_error_text(A.EHIP, "ctx.hip(150): hipMalloc failed", earlier)
    with pytest.raises(AssertionError, match="earlier error"):                        # the stale text of the ctx_scan exits
        A.check_error_text(A.ENOMEM, earlier, earlier)
    with pytest.raises(AssertionError, match="empty"):
        A.check_error_text(A.ENOMEM, "", earlier)
    with pytest.raises(AssertionError, match="does not name"):
        A.check_error_text(A.ENOMEM, "merge.hip(748): the books do not add up", earlier)
    A.check_fired(0)
    with pytest.raises(AssertionError, match="never made"):
        A.check_fired(3)


def test_check_untouched_descriptor_and_released():
    A.check_untouched(np.full(64, 0xFF, np.uint8))
    hits = np.full(4, 0xFFFFFFFF, np.uint32); hits[2] = 7
    with pytest.raises(AssertionError, match="the first at byte 8"):
        A.check_untouched(hits)
    A.check_descriptor_unchanged(b"\xa5" * 8, b"\xa5" * 8)
    with pytest.raises(AssertionError, match="descriptor changed"):
        A.check_descriptor_unchanged(b"\xa5" * 8, b"\xa5" * 7 + b"\x00")
    A.check_released(0, 0, 0, 0, 0x7f0000001000)
    with pytest.raises(AssertionError, match="gone"):                                 # the mutation of DESIGN.md section 6: cells still names the released buffer
        A.check_released(0x7f0000002000, 0, 0, 0, 0x7f0000001000)
    with pytest.raises(AssertionError, match="caller's to free"):
        A.check_released(0, 0, 0, 0, 0)


def test_entered_in_place_reads_the_build_counts():
    # iterations of three passes each: 1000 -> 400 (merged more than half: compacting), 400 -> 390 (less than half, the loop goes on: entered), 390 -> 389
    assert A.entered_in_place([1000, 900, 500, 400, 398, 395, 390, 390, 390], 389, 0.9999)
    assert not A.entered_in_place([1000, 900, 500], 400, 0.9999)                      # one iteration: nothing behind it
    assert not A.entered_in_place([1000, 700, 500, 400, 300, 200], 190, 0.9999)       # every iteration merges more than half


def test_the_fixture_scene():
    tris = A.fixture_scene()
    assert tris.shape == (3012, 12) and tris.dtype == np.float32 and np.isfinite(tris).all()
    small = np.abs(tris[:1500, 4:7]).max()
    assert small < 0.01 < np.abs(tris[1500:3000, 4:7]).max()                          # half the soup shrunk into the 3 % box
    assert tris[:1500, 0:3].min() >= 0.6 and tris[:1500, 0:3].max() <= 0.63 + 1e-6
    assert np.abs(tris[3000:, 4:7]).max() >= 5.0                                      # the wall quads
