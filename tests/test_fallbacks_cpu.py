"""The reach conditions of tests/test_fallbacks_gpu.py that need no GPU: the inputs of that file really cross the constants behind which the fall-back
branches lie.  The needle scenes hold more large primitives than count_top_refs / emit_top_refs have workgroups for; the expansion scenes' cells still grow
in the iterations where the GPU test moves the switch between listed and all-cells passes; the whole-lattice case has 12 800 tasks; and on that scene the
host's scatter by tasks and the definition agree independently of the device."""
import numpy as np
import pytest

import _distance as D
import _fallbacks as F


@pytest.mark.parametrize("m", F.NEEDLE_COUNTS)
def test_needle_scene_has_more_large_primitives_than_workgroups(m):
    """top level 8 x 8 x 8, shift 5; every needle's box covers at least 216 top-level cells (6 x 6 x 6), three times kCoopCells: rounding cannot matter"""
    from oracle import oracle as O
    tris = F.needle_scene(m)
    G = O.Grid.build(tris)
    assert G.dims == (8, 8, 8) and G.shift == 5
    covered = F.top_cells_covered(tris, G.dims, G.bbox_min, G.bbox_max)
    assert covered[2000:].min() >= 3 * F.COOP_CELLS
    large = F.large_primitives(tris, G.dims, G.bbox_min, G.bbox_max)
    assert large >= m and (large > F.BIG_BLOCKS) == (m > F.BIG_BLOCKS)


# cells whose box differs between expand(k) and expand(k - 1) from the fresh grid, k = 1 .. 6, as measured on the oracle (subset_only / precise):
#   soup4000       14 774 cells   12942  5184  1040   274    71   21   /  13081  5534  1202   384   116   34
#   soup1500_fine  81 431 cells   81385 77645 45962 14590  4590 1499   /  81392 78595 49763 16589  5746 2089
#   soup333_fine   18 831 cells   18821 17986 10798  3481   969  262   /  18822 18170 11585  4062  1273  430
#   clustered      14 914 cells   12370  6895  3220  1462   437  121   /  13240  9377  4158  2028   896  339
@pytest.mark.parametrize("subset_only", [True, False])
@pytest.mark.parametrize("name", sorted(F.EXPAND_SCENES))
def test_expansion_scenes_still_grow_where_the_switch_is_moved(name, subset_only):
    """iterations 2 .. 5 change cells in every scene, iterations 3 and 4 hundreds of them: a pass that took the wrong buffer there would be seen"""
    E = F.oracle_expansions(name, range(1, 6), subset_only)
    changed = {k: F.cells_differ(E[k], E[k - 1]) for k in range(2, 6)}
    assert all(c > 0 for c in changed.values()), changed
    assert changed[3] >= 100 and changed[4] >= 100, changed


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("fallbacks_host")
    return D.build_host(d), d


def test_whole_lattice_case_has_12800_tasks(host):
    exe, d = host
    tris, origin, size, n, band = F.whole_lattice_case()
    _, cnt = D.host_distance(exe, d, tris, origin, size, n, band, "scatter")
    assert cnt[0] == 200 and cnt[1] == 12800 and cnt[3] == 64 * 64 * 32, cnt
    assert D.TASK_VOXELS * 64 == 64 * 64 * 32               # 64 tasks per triangle: every box is the whole lattice


def test_host_scatter_by_tasks_equals_the_definition(host):
    """the whole-lattice scene at 16 x 16 x 8: the header's scatter with 64 voxels per task, the tasks last to first, against the definition over all pairs"""
    exe, d = host
    tris, origin, size, n, band = F.whole_lattice_case((16, 16, 8))
    want, cw = D.host_distance(exe, d, tris, origin, size, n, band, "brute")
    got, cg = D.host_distance(exe, d, tris, origin, size, n, band, "scatter", 64, True)
    D.assert_records_equal(got, want, "scatter T=64 reversed against the definition")
    assert cg[0] == 200 and cg[1] == 200 * 32 and cg[2] == cw[2] and cg[3] == cw[3] == 2048, (cg, cw)
    assert np.unique(want["id"]).size > 100 and (want["id"] >= 0).all()
