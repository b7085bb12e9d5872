"""tests/_gpu_case.py without a GPU: the assertions that eleven GPU test files share must be able to fail.  kernel_budget on canned listings; the lattice
table against entry points that accept one case each; the ctypes conversions; image_present, nearest_hit_unmoved and released_grid against a fake manager and a
fake api that record their calls."""
import ctypes as C
import types

import numpy as np
import pytest

import _gpu_case as G
from hagrid_amd import scene


# ---- kernel_budget ----------------------------------------------------------------------------------------------------------------------------------------
def listing(count, names):
    """the shape of what tools/count_kernels.py -v prints: a line per kernel, then the line that G.KERNEL_COUNT matches (made from the pattern itself)"""
    return "".join(f"  {n}(Args)\n" for n in names) + G.KERNEL_COUNT.replace(r"(\d+)", str(count)) + " libhagrid_amd.so\n"


def test_kernel_budget_passes_at_the_limit():
    assert G.MAX_KERNELS == 120
    G.kernel_budget(listing(120, ["a_kernel", "crossings_kernel", "b_kernel"]), one_each=("crossings_kernel",), absent=("bw_copy_kernel",))
    G.kernel_budget(listing(40, []))


@pytest.mark.parametrize("text,kw", [
    (listing(121, ["crossings_kernel"]), dict(one_each=("crossings_kernel",))),                         # one kernel too many
    (listing(120, ["crossings_kernel", "crossings_kernel"]), dict(one_each=("crossings_kernel",))),     # the named kernel twice
    (listing(120, ["a_kernel"]), dict(one_each=("crossings_kernel",))),                                 # ... and not at all
    (listing(120, ["a_kernel", "bw_copy_kernel"]), dict(absent=("bw_copy_kernel",))),                   # a kernel that must be gone
    ("no count at all\n", {}),
], ids=["121", "twice", "missing", "absent-present", "no-count"])
def test_kernel_budget_fails(text, kw):
    with pytest.raises(AssertionError):
        G.kernel_budget(text, **kw)


# ---- the lattice table ------------------------------------------------------------------------------------------------------------------------------------
def test_lattice_table_passes_where_everything_is_refused():
    seen = []
    G.assert_lattice_refused(lambda origin, size, n: seen.append((origin, size, n)) or G.EINVAL)
    assert len(seen) == len(G.LATTICES_REFUSED) == 19


@pytest.mark.parametrize("accepted", range(len(G.LATTICES_REFUSED)))
def test_lattice_table_fails_on_each_case_accepted(accepted):
    """an entry point that lets one lattice of the table through (status 0, or ERANGE in its place) is caught; compared by position: NaN != NaN"""
    for status in (0, G.ERANGE):
        calls = iter(range(len(G.LATTICES_REFUSED)))
        with pytest.raises(AssertionError):
            G.assert_lattice_refused(lambda origin, size, n: status if next(calls) == accepted else G.EINVAL)


def test_lattice_table_holds_what_the_product_refuses():
    """every case restated: check_lattice (hagrid_amd/csrc/trav_common.h) refuses a null array, a count <= 0, more than 2^31 - 1 voxels in the plane or in all, a size
    that is not positive and finite, an origin that is not finite -- and nothing in the table is a lattice it accepts"""
    def refused(origin, size, n):
        if origin is None or size is None or n is None:
            return True
        if min(n) <= 0 or n[0] * n[1] > 2 ** 31 - 1 or n[0] * n[1] * n[2] > 2 ** 31 - 1:
            return True
        return not all(0 < s < np.inf for s in size) or not all(np.isfinite(o) for o in origin)
    assert all(refused(*case) for case in G.LATTICES_REFUSED)
    assert not refused((0, 0, 0), (1, 1, 1), (2, 2, 2))


# ---- the ctypes conversions -------------------------------------------------------------------------------------------------------------------------------
def test_conversions():
    assert G.pod(None) is None and G.f3(None) is None and G.i3(None) is None and G.vp(None) is None
    f = G.f3(np.float32([0.5, -2.0, np.inf]))
    assert isinstance(f, C.c_float * 3) and list(f) == [0.5, -2.0, np.inf]
    assert np.isnan(G.f3((float("nan"), 0, 0))[0])
    i = G.i3(np.int64([1 << 30, -1, 4]))
    assert isinstance(i, C.c_int * 3) and list(i) == [1 << 30, -1, 4]
    assert isinstance(G.vp(0), C.c_void_p) and G.vp(0).value is None and G.vp(0x7F0000001000).value == 0x7F0000001000

    class Pod(C.Structure):
        _fields_ = [("shift", C.c_int)]
    grid = types.SimpleNamespace(pod=Pod(7))
    ref = G.pod(grid)
    assert ref is not None and ref._obj is grid.pod, "by reference: the entry point sees the grid's own structure"


# ---- the sequences, against fakes -------------------------------------------------------------------------------------------------------------------------
class FakeMem:
    """records the calls; image_bytes, order_state and the downloaded hits come from lists that the test fills (the last value repeats)"""
    def __init__(self, image_bytes=(4096,), order_state=((1, 2),), hits=None):
        self.calls, self.binning, self.options = [], 0, {}
        self._image, self._state, self._hits = list(image_bytes), list(order_state), list(hits or [])
        self.live = set()
        self._next = 0x1000

    @staticmethod
    def _take(values):
        return values.pop(0) if len(values) > 1 else values[0]

    def set_option(self, key, value):
        self.calls.append(("set_option", key, value)); self.options[key] = value

    def set_ray_binning(self, mode):
        self.calls.append(("set_ray_binning", mode)); self.binning = mode

    def image_bytes(self, grid):
        return self._take(self._image)

    def order_state(self, d_rays):
        return self._take(self._state)

    def alloc(self, nbytes):
        self._next += 0x1000; self.live.add(self._next); return self._next

    def upload(self, a):
        return self.alloc(a.nbytes)

    def free(self, p):
        self.live.remove(p)

    def one(self, p, nbytes):
        pass

    def synchronize(self):
        pass

    def download(self, p, dtype, count):
        return self._take(self._hits)


def fake_case(mem):
    api = types.SimpleNamespace(HIT_DTYPE=scene.HIT_DTYPE, calls=[])
    api.setup_traversal = lambda grid: api.calls.append(("setup_traversal", grid))
    api.traverse_grid = lambda grid, d_tris, d_rays, d_hits, n: api.calls.append(("traverse_grid", n))
    api.release_for_traversal = lambda grid: api.calls.append(("release_for_traversal", grid))
    api.build_all = lambda mem, d_tris, n: types.SimpleNamespace(freed=False, free=lambda: api.calls.append(("free",)))
    c = G.Case()
    c.api, c.mem, c.d_tris, c.tris = api, mem, 0x100, np.zeros((5, 12), np.float32)
    return c


GRID = types.SimpleNamespace(bbox_min=np.float32([0, 0, 0]), bbox_max=np.float32([1, 1, 1]))


def hits(ids):
    h = np.zeros(len(ids), dtype=scene.HIT_DTYPE)
    h["id"] = ids
    h["t"] = np.float32(1.5)
    return h


def test_image_present_sequence_and_exit_state():
    c = fake_case(FakeMem())
    with G.image_present(c, GRID):
        assert c.mem.options == {"traverse.image": 2} and c.api.calls == [("setup_traversal", GRID)] and c.mem.binning == 0
        c.mem.set_ray_binning(1)
    assert c.mem.binning == 0 and c.mem.options == {"traverse.image": 2}
    with G.image_present(c, GRID, binning=True):
        assert c.mem.binning == 1
    assert c.mem.binning == 0
    G.drop_image(fake_case(FakeMem(image_bytes=(0,))), GRID)


def test_image_present_fails_without_an_image_before_or_after():
    with pytest.raises(AssertionError):
        with G.image_present(fake_case(FakeMem(image_bytes=(0,))), GRID):
            pytest.fail("the body must not run without an image")
    c = fake_case(FakeMem(image_bytes=(4096, 0)))
    with pytest.raises(AssertionError, match="dropped the traversal image"):
        with G.image_present(c, GRID, binning=True):
            pass
    assert c.mem.binning == 0
    with pytest.raises(AssertionError):
        G.drop_image(fake_case(FakeMem(image_bytes=(4096,))), GRID)


def test_image_present_switches_binning_off_when_the_body_raises():
    c = fake_case(FakeMem())
    with pytest.raises(KeyError):
        with G.image_present(c, GRID):
            c.mem.set_ray_binning(1)
            raise KeyError("the body's own failure comes through")
    assert c.mem.binning == 0 and c.mem.calls[-1] == ("set_ray_binning", 0)


def test_nearest_hit_unmoved_passes_and_frees_its_buffers():
    h = hits([3, -1, 7])
    c = fake_case(FakeMem(hits=[h, h.copy()]))
    with G.nearest_hit_unmoved(c, GRID) as run:
        assert run.before is h and run.after is None and len(c.mem.live) == 2
    assert run.after is not None and not c.mem.live
    assert c.api.calls == [("traverse_grid", 64 * 64)] * 2
    c = fake_case(FakeMem(hits=[h, h.copy()]))
    with G.nearest_hit_unmoved(c, GRID, 0x5000, 3):                 # the caller's rays: not freed here
        assert len(c.mem.live) == 1
    assert c.api.calls == [("traverse_grid", 3)] * 2 and not c.mem.live


def test_nearest_hit_unmoved_fails_on_moved_hints_changed_hits_and_no_hit():
    h = hits([3, -1, 7])
    with pytest.raises(AssertionError, match="hints"):
        with G.nearest_hit_unmoved(fake_case(FakeMem(order_state=((1, 2), (1, 3)), hits=[h, h.copy()])), GRID):
            pass
    one_bit = h.copy()
    one_bit["t"][1] = np.nextafter(np.float32(1.5), np.float32(2))
    assert (one_bit.view(np.uint32) != h.view(np.uint32)).sum() == 1
    with pytest.raises(AssertionError):
        with G.nearest_hit_unmoved(fake_case(FakeMem(hits=[h, one_bit])), GRID):
            pass
    miss = hits([-1, -1, -1])
    with pytest.raises(AssertionError):
        with G.nearest_hit_unmoved(fake_case(FakeMem(hits=[miss, miss.copy()])), GRID):
            pass


def test_released_grid():
    c = fake_case(FakeMem())
    with G.released_grid(c) as g2:
        assert g2 is not None and c.mem.options == {"traverse.image": 2}
        assert [call[0] for call in c.api.calls] == ["setup_traversal", "release_for_traversal"] and c.api.calls[1][1] is g2
    assert c.api.calls[-1] == ("free",)
    c = fake_case(FakeMem(image_bytes=(0,)))                       # no image was made: nothing to release, the body is told
    with G.released_grid(c) as g2:
        assert g2 is None
    assert [call[0] for call in c.api.calls] == ["setup_traversal", "free"]
    c = fake_case(FakeMem())
    own = c.api.build_all(c.mem, c.d_tris, 5)
    with pytest.raises(KeyError):
        with G.released_grid(c, own) as g2:
            assert g2 is own
            raise KeyError
    assert c.api.calls[-1] == ("free",), "freed when the body raises, too"


def test_assert_totals_added():
    class Mem(FakeMem):
        def upload(self, a):
            self.tot = a.copy(); return self.alloc(a.nbytes)

        def download(self, p, dtype, count):
            return self.tot[:count]

    tot = np.int64([4, 10, 0, 7])
    mem = Mem()
    G.assert_totals_added(lambda d_tot: mem.tot.__iadd__(tot), mem, tot)
    assert not mem.live
    with pytest.raises(AssertionError):                             # a launch that overwrites the counters
        G.assert_totals_added(lambda d_tot: None, Mem(), tot)
