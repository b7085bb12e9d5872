"""The scan-line fill on the GPU (hagrid_fill_lattice, the row form of the kernel of hagrid_amd/csrc/crossings.hip): every lattice of the fixture
tests/golden/fill_lattice.npz on Cell and SmallCell grids built on the device, every axis mask and both vote rules, records and counters null and given, bit
for bit; the counters against the host walk's; row counts around the wavefront; output and workspace at every alignment the packed stores meet; a traversal
image present and ray binning on; one axis with a null workspace; api.solid_voxels and the snippets of INTEGRATION.md on torch's stream; a C++ program through
the shim; every argument error; the kernel budget.  Every compared output comes from a poisoned, guarded buffer (tests/_poison.py).
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import sys

import numpy as np
import pytest

import _crossings as X
import _fill_lattice as FL
import _gpu_case as G
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

WINDING = 1


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FL.FIXTURE))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("fill_lattice_host_gpu")
    return FL.build_host(d), d


@pytest.fixture(scope="module", params=FL.SCENES)
def case(request):
    """one scene of the fixture: Cell and SmallCell grids built on the device"""
    c = G.open_case(request.param, FL.make_tris(request.param))
    c.lattices = FL.lattices(c.name, c.tris)
    yield c
    c.mem.close()


def run_fill(c, grid, origin, size, n, axes=7, winding=False, records=True, counters=True, workspace=True, shift_inside=0, shift_work=0):
    """what FL.host_fill returns, from the device: "inside" int32 per voxel, "records" (rows, 4) uint32 or None, "totals" int64[5] or None.  shift_inside (a
    multiple of 4) and shift_work: bytes by which the output and the workspace are moved off their allocation's alignment; the bytes in front stay poison."""
    mem = c.mem
    voxels = int(np.prod([int(v) for v in n]))
    rows = FL.rows_of_mask(n, axes or 7).size
    d_in = P.alloc_out(mem, 4 * voxels + shift_inside)
    d_ws = P.alloc_out(mem, voxels + shift_work) if workspace else 0
    d_rec = P.alloc_out(mem, 16 * rows) if records else 0
    d_tot = 0
    if counters:
        d_tot = mem.alloc(40); mem.zero(d_tot, 40)
    c.api.fill_lattice(grid, c.d_tris, origin, size, n, d_in + shift_inside, axes=axes, workspace=d_ws + shift_work if workspace else 0, records=d_rec, counters=d_tot,
                       flags=WINDING if winding else 0)
    mem.synchronize()
    raw = P.fetch(mem, d_in, np.uint8, 4 * voxels + shift_inside)
    assert (raw[:shift_inside] == 0xFF).all(), "written in front of the output"
    out = {"inside": raw[shift_inside:].view(np.int32).copy(), "records": None, "abstained": None, "totals": None}
    mem.free(d_in)
    if workspace:
        raw = P.fetch(mem, d_ws, np.uint8, voxels + shift_work)              # (the guard behind the workspace; its content is unspecified)
        assert (raw[:shift_work] == 0xFF).all(), "written in front of the workspace"
        mem.free(d_ws)
    if records:
        out["records"] = P.fetch(mem, d_rec, np.uint32, 4 * rows).reshape(rows, 4).copy()
        mem.free(d_rec)
    if counters:
        out["totals"] = mem.download(d_tot, np.int64, 5)
        mem.free(d_tot)
    return out


@pytest.mark.parametrize("compress", [False, True])
def test_device_equals_the_fixture(case, fixture, compress):
    """every lattice, every axis mask, both rules: inside and records are the fixture's; rows and abstaining rows are counted"""
    c = case
    for key, origin, size, n in c.lattices:
        for winding in (False, True):
            for mask in FL.MASKS:
                want = FL.fixture_case(fixture, key, mask, winding)
                got = run_fill(c, c.grids[compress], origin, size, n, mask, winding)
                FL.assert_fill_equal(got, want, f"{key} compress={compress} axes={mask} winding={winding}")
                assert got["totals"][0] == want["abstained"].size and got["totals"][4] == want["abstained"].sum()
        got = run_fill(c, c.grids[compress], origin, size, n, 0, True)
        FL.assert_fill_equal(got, FL.fixture_case(fixture, key, 7, True), f"{key}: axes = 0 means 7")


def test_records_and_counters_null(case, fixture):
    c = case
    for key, origin, size, n in c.lattices:
        for mask in (7, 3, 4):
            got = run_fill(c, c.grids[True], origin, size, n, mask, True, records=False, counters=False)
            assert got["records"] is None and got["totals"] is None
            FL.assert_fill_equal(got, FL.fixture_case(fixture, key, mask, True), f"{key} axes={mask}: records and counters null")


def test_one_axis_needs_no_workspace(case, fixture):
    c = case
    key, origin, size, n = c.lattices[0]
    for mask in (1, 2, 4):
        for winding in (False, True):
            got = run_fill(c, c.grids[False], origin, size, n, mask, winding, workspace=False)
            FL.assert_fill_equal(got, FL.fixture_case(fixture, key, mask, winding), f"{key} axes={mask}: null workspace")


def test_every_alignment_of_output_and_workspace(case, fixture):
    """rows along x store four voxels at a time where the address allows: the output 0, 4, 8 and 12 bytes off a 16-byte boundary, the workspace 0 .. 3 bytes
    off a dword"""
    c = case
    for key, origin, size, n in c.lattices:
        for k in range(4):
            for mask, winding in ((7, True), (1, False), (3, False)):
                got = run_fill(c, c.grids[k % 2 == 1], origin, size, n, mask, winding, shift_inside=4 * k, shift_work=(k + 1) % 4)
                FL.assert_fill_equal(got, FL.fixture_case(fixture, key, mask, winding), f"{key} axes={mask}: output {4 * k} bytes, workspace {(k + 1) % 4} bytes off")


@pytest.mark.parametrize("compress", [False, True])
def test_counters_equal_the_host_walk(case, host, compress):
    """the five batch totals against the host walk over the device's own grid; they are ADDED to"""
    c = case
    exe, d = host
    grid = c.grids[compress]
    arrays = grid.download(c.mem)
    key, origin, size, n = c.lattices[0]
    for mask, winding in ((7, False), (6, True)):
        got = run_fill(c, grid, origin, size, n, mask, winding)
        w = FL.host_fill(exe, d, c.tris, origin, size, n, mask, winding, grid=arrays, page=8)
        assert got["totals"].tolist() == w["totals"].tolist() and (got["totals"][:4] > 0).all()
        FL.assert_fill_equal(got, w, f"{key} compress={compress} against the host walk over the device's grid")
    mem = c.mem
    voxels = int(np.prod(n))
    d_in = mem.alloc(4 * voxels); d_ws = mem.alloc(voxels)
    G.assert_totals_added(lambda d_tot: c.api.fill_lattice(grid, c.d_tris, origin, size, n, d_in, axes=6, workspace=d_ws, counters=d_tot, flags=WINDING), mem, got["totals"])
    mem.free(d_in); mem.free(d_ws)


def test_row_counts_around_the_wavefront(host):
    """lattices with 1, 63, 64 and 65 rows along an axis, against the host's brute force: the tail of a wavefront writes nothing"""
    exe, d = host
    c = G.upload_case(FL.make_tris("boxes"))
    grid = c.api.build_all(c.mem, c.d_tris, c.tris.shape[0], compress=True)
    origin, size = np.float32([-0.3, -0.2, -0.1]), np.float32([0.21, 0.17, 0.19])
    for n in ((8, 8, 1), (9, 7, 1), (5, 13, 1), (1, 64, 3), (65, 1, 2), (1, 1, 130)):
        for mask, winding in ((7, True), (5, False)):
            got = run_fill(c, grid, origin, size, n, mask, winding)
            FL.assert_fill_equal(got, FL.host_fill(exe, d, c.tris, origin, size, n, mask, winding), f"boxes {n} axes={mask}")
            assert got["totals"][0] == FL.rows_of_mask(n, mask).size
    grid.free()
    c.mem.close()


def test_image_and_binning_are_ignored_and_survive(case, fixture):
    c = case
    grid = c.grids[False]
    key, origin, size, n = c.lattices[0]
    with G.image_present(c, grid, binning=True):
        got = run_fill(c, grid, origin, size, n, 7, True)
    FL.assert_fill_equal(got, FL.fixture_case(fixture, key, 7, True), f"{key} image present, binning on")


def test_neighbours_give_the_bits_they_gave(case):
    """hagrid_inside_lattice over the fill's lattice after fills on the same context: scene.points_inside, as before"""
    c = case; mem = c.mem
    key, origin, size, n = c.lattices[-1]
    voxels = int(np.prod(n))
    run_fill(c, c.grids[True], origin, size, n, 7, True)
    d_in = P.alloc_out(mem, 4 * voxels)
    c.api.inside_lattice(c.grids[True], c.d_tris, origin, size, n, d_in)
    mem.synchronize()
    got = P.fetch(mem, d_in, np.int32, voxels)
    mem.free(d_in)
    assert (got == scene.points_inside(c.tris, scene.lattice_centres(origin, size, n))["inside"]).all()


def test_solid_voxels_from_torch_tensors(fixture):
    """api.solid_voxels on torch's stream, and the signed-distance snippet of INTEGRATION.md: the sign from the fill, the distance from closest_points"""
    import torch
    from hagrid_amd import api
    tris = FL.make_tris("solids")
    key, origin, size, n = FL.lattices("solids", tris)[0]
    nx, ny, nz = (int(v) for v in n)
    mem = api.MemManager(keep=True)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_tris = torch.from_numpy(tris).cuda()
            grid = api.build_all(mem, t_tris.data_ptr(), tris.shape[0])
            solid = api.solid_voxels(grid, t_tris, origin, size, n)
            assert solid.dtype == torch.int32 and tuple(solid.shape) == (nz, ny, nx)
            parity_z = api.solid_voxels(grid, t_tris, origin, size, n, axes=4, winding=False)
            # INTEGRATION.md, signed distance on a lattice and solid voxelization
            fill = solid
            centres = torch.from_numpy(scene.lattice_centres(origin, size, n).view(np.float32).reshape(-1, 4)).cuda()
            res = torch.empty((nz * ny * nx, 8), dtype=torch.float32, device="cuda")
            api.closest_points(grid, t_tris.data_ptr(), centres.data_ptr(), res.data_ptr(), nz * ny * nx)
            sdf = (torch.sqrt(res[:, 3]) * (1 - 2 * (fill.reshape(-1) == 1).int())).reshape(nz, ny, nx)
            ids = torch.empty(nz * ny * nx, dtype=torch.int32, device="cuda")
            cnt = torch.empty(nz * ny * nx, dtype=torch.int32, device="cuda")
            api.voxelize(grid, t_tris.data_ptr(), origin, size, (nx, ny, nz), 1, ids.data_ptr(), cnt.data_ptr(), flags=api.OVERLAP_ANY)
            voxels = (cnt.reshape(nz, ny, nx) > 0) | (fill == 1)
            assert voxels.dtype == torch.bool and bool((voxels | (fill != 1)).all()) and int(voxels.sum()) > int((fill == 1).sum())
            got = solid.cpu().numpy(); got_z = parity_z.cpu().numpy(); got_sdf = sdf.cpu().numpy()
            grid.free()
        stream.synchronize()
    finally:
        mem.use_stream(None)
    mem.close()
    assert (got.reshape(-1) == fixture[key + "_inside"][1, 6]).all() and (got_z.reshape(-1) == fixture[key + "_inside"][0, 3]).all()
    truth, dist = FL.solids_truth(FL.centres(origin, size, n))
    far = dist > FL.NEAR
    assert ((got_sdf.reshape(-1) < 0) == (truth == 1))[far].all()


def test_cpp_program_through_the_shim(tmp_path):
    import _subproc
    r = _subproc.check([G.build_shim("fill_lattice", tmp_path), "40"], timeout=120)
    sys.stdout.write(r.stdout)
    assert " 0 mismatches vs host fill_row, 0 records differ, 0 mismatches vs the boxes" in r.stdout, r.stdout


def test_errors_leave_the_context_working(case, fixture):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    key, origin, size, n = c.lattices[0]
    voxels = int(np.prod(n))
    rows = sum(FL.row_counts(n))
    d_in = mem.alloc(4 * voxels + 64); d_ws = mem.alloc(voxels + 64); d_rec = mem.alloc(16 * rows + 64); d_tot = mem.alloc(64)
    EINVAL = G.EINVAL
    vp = G.vp

    def call(g=grid, tris=c.d_tris, o=origin, s=size, k=n, axes=7, inside=d_in, work=d_ws, records=d_rec, counters=d_tot, flags=0, ctx=mem._ctx):
        return L.hagrid_fill_lattice(ctx, G.pod(g), vp(tris), G.f3(o), G.f3(s), G.i3(k), axes, vp(inside), vp(work), vp(records), vp(counters), flags)

    assert call() == 0 and call(flags=WINDING) == 0 and call(records=0, counters=0) == 0 and call(axes=4, work=0) == 0 and call(axes=0) == 0
    # a null context, a null grid, null buffers
    assert call(ctx=None) == EINVAL
    assert call(g=None) == EINVAL and b"grid" in L.hagrid_last_error(mem._ctx)
    assert call(tris=0) == EINVAL and call(inside=0) == EINVAL and b"null" in L.hagrid_last_error(mem._ctx)
    # the workspace is needed with more than one axis
    for axes in (0, 3, 5, 6, 7):
        assert call(axes=axes, work=0) == EINVAL and b"workspace" in L.hagrid_last_error(mem._ctx)
    # an axes bit beyond 7
    for axes in (8, 15, 1 << 31):
        assert call(axes=axes) == EINVAL and b"axes" in L.hagrid_last_error(mem._ctx)
    # misaligned buffers
    assert call(inside=d_in + 2) == EINVAL and call(inside=d_in + 1) == EINVAL and b"aligned" in L.hagrid_last_error(mem._ctx)
    assert call(tris=c.d_tris + 4) == EINVAL and call(records=d_rec + 8) == EINVAL and call(counters=d_tot + 4) == EINVAL and b"aligned" in L.hagrid_last_error(mem._ctx)
    assert call(inside=d_in + 4, work=d_ws + 1) == 0, "inside needs 4 bytes, the workspace none"
    # the lattice: a count of zero is not possible; null arrays
    G.assert_lattice_refused(lambda o, s, k: call(o=o, s=s, k=k))
    assert call(k=(4, 4, 0)) == EINVAL and b"voxel" in L.hagrid_last_error(mem._ctx)
    # an unknown flag
    for flags in (2, 4, 1 << 31):
        assert call(flags=flags) == EINVAL and b"flag" in L.hagrid_last_error(mem._ctx)
    with pytest.raises(api.HagridError, match="workspace"):
        api.fill_lattice(grid, c.d_tris, origin, size, n, d_in)
    with pytest.raises(api.HagridError, match="aligned"):
        api.fill_lattice(grid, c.d_tris, origin, size, n, d_in + 2, axes=1)
    # "traverse.id_is_steps" = 1
    mem.set_option("traverse.id_is_steps", 1)
    try:
        with pytest.raises(api.HagridError, match="id_is_steps"):
            api.fill_lattice(grid, c.d_tris, origin, size, n, d_in, workspace=d_ws)
    finally:
        mem.set_option("traverse.id_is_steps", 0)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.fill_lattice(g2, c.d_tris, origin, size, n, d_in, workspace=d_ws)
    mem.free(d_in); mem.free(d_ws); mem.free(d_rec); mem.free(d_tot)
    got = run_fill(c, grid, origin, size, n, 7, True)
    FL.assert_fill_equal(got, FL.fixture_case(fixture, key, 7, True), f"{key} after the refused calls")


def test_overflowed_centres_vote_outside():
    """a lattice whose centres overflow float32: the rows are not admissible, have no crossings and vote 0; nothing is read or written out of bounds"""
    c = G.upload_case(FL.make_tris("boxes"))
    grid = c.api.build_all(c.mem, c.d_tris, c.tris.shape[0])
    n = (3, 2, 2)
    got = run_fill(c, grid, np.float32([3e38, 0.1, 0.1]), np.float32([3e38, 0.2, 0.2]), n, 7, True)
    want = scene.fill_lattice(c.tris, np.float32([3e38, 0.1, 0.1]), np.float32([3e38, 0.2, 0.2]), n, 7, True)
    assert (got["inside"] == want["inside"]).all() and (got["inside"] == 0).all()
    X.assert_records_equal(got["records"], want["records"], "overflowed centres")
    grid.free()
    c.mem.close()


def test_kernel_budget():
    """the row form is a mode of the one crossings kernel, not a kernel of its own"""
    from hagrid_amd import lib
    assert "hagrid_fill_lattice" in lib.SIGNATURES
    G.kernel_budget(G.kernel_listing(), one_each=("crossings_kernel",))         # crossing queries are ONE kernel
