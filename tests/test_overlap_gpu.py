"""Box-overlap queries on the GPU (hagrid_amd/csrc/overlap.hip): the device's ids and counts against the fixture tests/golden/overlap.npz on Cell and
SmallCell grids built on the device, for k = 1, 2, 3, 5, 8, with a traversal image present and ray binning on, with counts null; the batch totals against
the host walk's; batch tails; ANY; the lattice form; a larger live case against the host walk; the frame loop from torch tensors on torch's stream; a C++
program through the shim; every argument error; the kernel budget.
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import sys

import numpy as np
import pytest

import _gpu_case as G
import _overlap as V
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(V.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_host_gpu")
    return V.build_host(d), d


@pytest.fixture(scope="module", params=V.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, the boxes uploaded"""
    c = G.open_case(request.param, V.make_tris(request.param))
    c.fixture = fixture
    c.boxes = V.scene_boxes(fixture, c.name, c.tris)
    c.sizes = fixture[c.name + "_sizes"]
    c.n = c.boxes.shape[0]
    c.d_boxes = c.mem.upload(c.boxes)
    c.unb = V.unbounded_boxes(c.tris, V.NUM_UNBOUNDED, V.BOX_SEED + 200 + V.SCENES.index(c.name))
    assert V.box_sum(c.unb) == int(fixture[c.name + "_unb_box_sum"])
    c.d_unb = c.mem.upload(c.unb)
    c.grid_box = scene.grid_box(c.tris)
    for g in c.grids.values():
        assert (g.bbox_min.view(np.uint32) == c.grid_box[0].view(np.uint32)).all() and (g.bbox_max.view(np.uint32) == c.grid_box[1].view(np.uint32)).all(), "the fixture's grid box"
    yield c
    c.mem.close()


def run_overlap(c, grid, d_boxes, n, k, flags=0, counts=True, counters=False, d_tris=None, lattice=None):
    """(ids (n, k), counts or None[, the four batch totals]); the outputs are poisoned first and guarded"""
    mem = c.mem
    d_ids = P.alloc_out(mem, 4 * k * n)
    d_cnt = P.alloc_out(mem, 4 * n) if counts else 0
    d_tot = 0
    if counters:
        d_tot = mem.alloc(32); mem.zero(d_tot, 32)
    if lattice is None:
        c.api.overlap_boxes(grid, d_tris or c.d_tris, d_boxes, n, k, d_ids, d_cnt, d_tot, flags)
    else:
        c.api.voxelize(grid, d_tris or c.d_tris, lattice[0], lattice[1], lattice[2], k, d_ids, d_cnt, d_tot, flags)
    mem.synchronize()
    out = [P.fetch(mem, d_ids, np.int32, k * n).reshape(n, k).copy(), None]
    mem.free(d_ids)
    if counts:
        out[1] = P.fetch(mem, d_cnt, np.int32, n).copy()
        mem.free(d_cnt)
    if counters:
        out.append(mem.download(d_tot, np.int64, 4))
        mem.free(d_tot)
    return out


@pytest.mark.parametrize("compress", [False, True])
def test_device_results_equal_the_fixture(case, compress):
    """every box, k = 1, 2, 3, 5 and 8 (k = 8 is the path of two 16-byte stores per box, the others the path of 4-byte stores), and k = 4 (one 16-byte
    store) from the first 8 ids of the fixture as well; the 384 boxes with infinite bounds likewise"""
    c = case
    c.mem.set_option("traverse.image", 0)
    for k in V.KS + (4,):
        ids, counts = run_overlap(c, c.grids[compress], c.d_boxes, c.n, k)
        want_ids, want_counts = V.expected(c.fixture, c.name, k)
        V.assert_answers_equal(ids, counts, want_ids, want_counts, f"{c.name} compress={compress} k={k}")
        ids, counts = run_overlap(c, c.grids[compress], c.d_unb, V.NUM_UNBOUNDED, k)
        want_ids, want_counts = V.expected(c.fixture, c.name + "_unb", k)
        V.assert_answers_equal(ids, counts, want_ids, want_counts, f"{c.name} compress={compress} k={k}, infinite bounds")
    c.mem.set_option("traverse.image", 2)


@pytest.mark.parametrize("compress", [False, True])
def test_image_binning_and_null_counts(case, compress):
    """a traversal image and ray binning are ignored and survive; counts may be null"""
    c = case; mem = c.mem
    grid = c.grids[compress]
    want_ids, want_counts = V.expected(c.fixture, c.name, 5)
    with G.image_present(c, grid):
        ids, counts = run_overlap(c, grid, c.d_boxes, c.n, 5)
        V.assert_answers_equal(ids, counts, want_ids, want_counts, f"{c.name} image present")
        mem.set_ray_binning(1)
        ids, counts = run_overlap(c, grid, c.d_boxes, c.n, 5, counts=False)
        assert counts is None
        V.assert_answers_equal(ids, None, want_ids, None, f"{c.name} binning set, counts null")


@pytest.mark.parametrize("compress", [False, True])
def test_batch_totals_equal_the_host_walk(case, host, compress):
    c = case
    exe, d = host
    grid = c.grids[compress]
    arrays = grid.download(c.mem)
    for k, flags in ((1, 0), (8, 0), (1, c.api.OVERLAP_ANY)):
        ids, counts, tot = run_overlap(c, grid, c.d_boxes, c.n, k, flags=flags, counters=True)
        w_ids, w_counts, totals = V.host_walk(exe, d, arrays, c.tris, c.boxes, k, any_=bool(flags))
        V.assert_answers_equal(ids, counts, w_ids, w_counts, f"{c.name} compress={compress} k={k} flags={flags} against the host walk over the device's grid")
        assert tot.tolist() == [c.n, int(totals[:, 0].astype(np.int64).sum()), int(totals[:, 1].astype(np.int64).sum()), int(totals[:, 2].astype(np.int64).sum())]
        assert tot[1] > 0 and tot[2] > 0 and tot[3] > 0
    # the totals are ADDED: a second launch doubles them
    d_ids = c.mem.alloc(4 * c.n)
    G.assert_totals_added(lambda d_tot: c.api.overlap_boxes(grid, c.d_tris, c.d_boxes, c.n, 1, d_ids, 0, d_tot, c.api.OVERLAP_ANY), c.mem, tot)
    c.mem.free(d_ids)


def test_batch_tails(case):
    """batches of 1, 63, 65 and 4096 - 37 boxes, at an offset into the box buffer: the tail of a wavefront writes nothing"""
    c = case
    grid = c.grids[True]
    c.api.overlap_boxes(grid, c.d_tris, 0, 0, 3, 0)                 # no boxes: nothing is launched, null buffers are fine
    c.api.overlap_boxes(grid, 0, 0, 0, 8, 0, 0, 0)
    for n, first in ((1, 0), (63, 5), (65, 2040), (V.NUM_BOXES - 37, 37)):
        for k in (3, 8):
            ids, counts = run_overlap(c, grid, c.d_boxes + 32 * first, n, k)
            want_ids, want_counts = V.expected(c.fixture, c.name, k)
            V.assert_answers_equal(ids, counts, want_ids[first:first + n], want_counts[first:first + n], f"{c.name} n={n} first={first} k={k}")


@pytest.mark.parametrize("compress", [False, True])
def test_any(case, compress):
    """id >= 0 exactly where |S| > 0, and the returned id meets its box and respects `first`"""
    c = case
    ids, counts = run_overlap(c, c.grids[compress], c.d_boxes, c.n, 1, flags=c.api.OVERLAP_ANY)
    got = ids[:, 0]
    assert ((got >= 0) == (c.sizes > 0)).all() and (counts == (c.sizes > 0)).all()
    hit = got >= 0
    assert hit.sum() > 1000 and (got[~hit] == -1).all()
    assert scene.overlap_pairs(c.tris[got[hit]], scene.clip_boxes(c.boxes, *c.grid_box)[hit]).all()
    assert (got[hit] >= c.boxes[hit, 3].view(np.int32)).all()
    ids, counts = run_overlap(c, c.grids[compress], c.d_unb, V.NUM_UNBOUNDED, 1, flags=c.api.OVERLAP_ANY)
    usz = c.fixture[c.name + "_unb_sizes"]
    assert ((ids[:, 0] >= 0) == (usz > 0)).all() and (counts == (usz > 0)).all()
    hit = ids[:, 0] >= 0
    assert scene.overlap_pairs(c.tris[ids[hit, 0]], scene.clip_boxes(c.unb, *c.grid_box)[hit]).all()


def test_lattice(case):
    """a 33 x 17 x 9 lattice over the scene box enlarged a little: the device's boxes are scene.lattice_boxes's boxes"""
    c = case
    lo, hi = scene.tris_bbox(c.tris)
    ext = hi - lo
    n = (33, 17, 9)
    origin = (lo - np.float32(0.03) * ext).astype(np.float32)
    size = ((ext * np.float32(1.06)) / np.float32(n)).astype(np.float32)
    boxes = scene.lattice_boxes(origin, size, n)
    nv = boxes.shape[0]
    want = scene.overlap_boxes(c.tris, boxes, k=V.KMAX, grid=c.grid_box)
    assert (want["sizes"] == 0).any() and (want["sizes"] > V.KMAX).any()
    for compress, k in ((False, 8), (True, 3)):
        ids, counts = run_overlap(c, c.grids[compress], 0, nv, k, lattice=(origin, size, n))
        V.assert_answers_equal(ids, counts, want["ids"][:, :k], np.minimum(want["sizes"], k + 1).astype(np.int32), f"{c.name} lattice compress={compress} k={k}")
    ids, counts = run_overlap(c, c.grids[True], 0, nv, 1, flags=c.api.OVERLAP_ANY, lattice=(origin, size, n))
    assert ((ids[:, 0] >= 0) == (want["sizes"] > 0)).all() and (counts == (want["sizes"] > 0)).all()


def test_larger_live_case(tmp_path):
    """100 000 triangles, 65 536 boxes (0.5 % to 4 % of the diagonal, near the surface and uniform, some paged, one in 64 with an infinite bound, in one shuffled batch): the device's answers
    against the host walk over the SAME grid arrays (downloaded), batch totals included, and against the numpy statement for the first 128 boxes"""
    from hagrid_amd import api
    tris = scene.make_soup(100000)
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    n = 65536
    u = scene._uniform_rows(77, n, 2)
    edge = (np.float32(0.005) * diag) * (np.float32(1.0) + np.float32(7.0) * u[:, 0] * u[:, 0])
    b = V.boxes_around(np.concatenate([scene.make_points_near_surface(tris, lo, hi, n // 2, 11), scene.make_points_uniform(lo, hi, n // 2, 12)]), edge.astype(np.float32))
    b[::16, 3] = (u[::16, 1] * np.float32(tris.shape[0])).astype(np.int32).view(np.float32)
    for i in range(7, n, 64):
        f = (i // 64) % 6
        b[i, (0, 1, 2, 4, 5, 6)[f]] = -np.inf if f < 3 else np.inf
    b = np.ascontiguousarray(b[np.random.default_rng(5).permutation(n)])
    c = G.upload_case(tris); mem = c.mem
    d_boxes = mem.upload(b)
    exe = V.build_host(tmp_path)
    for compress, k in ((False, 8), (True, 2)):
        grid = api.build_all(mem, c.d_tris, tris.shape[0], compress=compress)
        ids, counts, tot = run_overlap(c, grid, d_boxes, n, k, counters=True)
        w_ids, w_counts, totals = V.host_walk(exe, tmp_path, grid.download(mem), tris, b, k)
        V.assert_answers_equal(ids, counts, w_ids, w_counts, f"soup 100k compress={compress} against the host walk")
        assert tot.tolist() == [n, int(totals[:, 0].sum()), int(totals[:, 1].sum()), int(totals[:, 2].sum())]
        if not compress:
            want = scene.overlap_boxes(tris, b[:128], k=k, grid=(grid.bbox_min, grid.bbox_max))
            V.assert_answers_equal(ids[:128], counts[:128], want["ids"], want["counts"], "soup 100k against the statement")
            assert (w_counts == k + 1).any() and (w_counts == 0).any() and (w_counts > 0).sum() > n // 2
            assert totals[:, 1].mean() < tris.shape[0] / 10
        grid.free()
    mem.close()


def test_frame_loop_from_torch_tensors():
    """the frame loop of api.MeshScene on torch's stream: assemble -> build -> query with boxes, ids, counts and totals in torch tensors; torch rewrites the
    vertices in place; assemble -> build -> query again: every answer is the statement's on the triangles of that frame"""
    import torch
    from hagrid_amd import api
    V_, F = scene.make_stadium_mesh(0.05)
    V_ = np.ascontiguousarray(V_, np.float32); F = np.ascontiguousarray(F, np.int32)
    nt = F.shape[0]
    mem = api.MemManager(keep=True)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            tV = torch.from_numpy(V_).cuda(); tF = torch.from_numpy(F).cuda()
            t_tris = torch.zeros((nt, 12), dtype=torch.float32, device="cuda")
            ms = api.MeshScene(mem, [(tV.data_ptr(), V_.shape[0], tF.data_ptr(), nt)])
            for frame in range(2):
                if frame == 1:
                    V_ = (V_ * np.float32([1.0, 1.25, 0.8]) + np.float32(0.05) * np.sin(3.0 * V_[:, [1, 2, 0]]).astype(np.float32)).astype(np.float32)
                    tV.copy_(torch.from_numpy(V_))
                ms.assemble(0, t_tris.data_ptr())
                grid = api.build_all(mem, t_tris.data_ptr(), nt)
                tris = t_tris.cpu().numpy()
                lo, hi = scene.tris_bbox(tris)
                diag = scene.bbox_diagonal(lo, hi)
                b = V.boxes_around(V.mixed_centres(tris, lo, hi, 1000, 21 + frame), np.float32(0.03) * diag)
                b[::50, 0] = -np.inf; b[25::50, 5] = np.inf      # some boxes without a bound
                t_boxes = torch.from_numpy(b).cuda()
                t_ids = torch.full((b.shape[0], 4), -7, dtype=torch.int32, device="cuda")
                t_cnt = torch.full((b.shape[0],), -7, dtype=torch.int32, device="cuda")
                t_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
                api.overlap_boxes(grid, t_tris.data_ptr(), t_boxes.data_ptr(), b.shape[0], 4, t_ids.data_ptr(), t_cnt.data_ptr(), t_tot.data_ptr())
                occupied = (t_cnt > 0).sum()                          # torch work on the same stream, after the launch
                ids = t_ids.cpu().numpy(); cnt = t_cnt.cpu().numpy(); tot = t_tot.cpu().numpy()
                want = scene.overlap_boxes(tris, b, k=4, grid=(grid.bbox_min, grid.bbox_max))
                V.assert_answers_equal(ids, cnt, want["ids"], want["counts"], f"frame {frame}")
                assert int(occupied) == int((want["sizes"] > 0).sum()) > 500 and tot[0] == b.shape[0] and tot[2] > 0
                # surface voxelization into a torch tensor
                n = (16, 12, 8)
                size = ((hi - lo) / np.float32(n)).astype(np.float32)
                t_vox = torch.full((n[2], n[1], n[0]), -7, dtype=torch.int32, device="cuda")
                api.voxelize(grid, t_tris.data_ptr(), lo, size, n, 1, t_vox.data_ptr(), flags=api.OVERLAP_ANY)
                vox = (t_vox >= 0).cpu().numpy().reshape(-1)
                assert (vox == (scene.overlap_boxes(tris, scene.lattice_boxes(lo, size, n), k=1, grid=(grid.bbox_min, grid.bbox_max))["sizes"] > 0)).all() and vox.any() and not vox.all()
                grid.free()
            stream.synchronize()
            ms.close()
    finally:
        mem.use_stream(None)
    mem.close()


def test_cpp_program_through_the_shim(tmp_path):
    import _subproc
    r = _subproc.check([G.build_shim("overlap", tmp_path), "20000", "1000"], timeout=120)
    sys.stdout.write(r.stdout)
    assert " 0 mismatches vs host brute force" in r.stdout and " 0 mismatches in the lattice form" in r.stdout, r.stdout


def test_errors_leave_the_context_working(case):
    c = case; api, mem = c.api, c.mem
    grid = c.grids[False]
    L = mem._L
    d_ids = mem.alloc(4 * 8 * c.n + 64)
    d_cnt = mem.alloc(4 * c.n + 64)
    d_tot = mem.alloc(64)
    EINVAL = G.EINVAL
    ANY = api.OVERLAP_ANY
    vp = G.vp

    def call(g, tris, boxes, n, k, ids, counts=0, counters=0, flags=0):
        return L.hagrid_overlap_boxes(mem._ctx, G.pod(g), vp(tris), vp(boxes), n, k, vp(ids), vp(counts), vp(counters), flags)

    def lattice(g, origin, size, n, k, ids, counts=0, counters=0, flags=0, tris=None):
        return L.hagrid_overlap_lattice(mem._ctx, G.pod(g), vp(c.d_tris if tris is None else tris), G.f3(origin), G.f3(size), G.i3(n), k, vp(ids), vp(counts), vp(counters), flags)

    assert call(grid, c.d_tris, c.d_boxes, c.n, 8, d_ids, d_cnt, d_tot) == 0
    assert call(None, c.d_tris, c.d_boxes, c.n, 8, d_ids) == EINVAL and b"grid" in L.hagrid_last_error(mem._ctx)
    for k in (0, -1, 9, 1 << 20):
        assert call(grid, c.d_tris, c.d_boxes, c.n, k, d_ids) == EINVAL and b"k must" in L.hagrid_last_error(mem._ctx)
        assert lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), k, d_ids) == EINVAL
    for k in (2, 8):
        assert call(grid, c.d_tris, c.d_boxes, c.n, k, d_ids, flags=ANY) == EINVAL and b"k = 1" in L.hagrid_last_error(mem._ctx)
        assert lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), k, d_ids, flags=ANY) == EINVAL
    assert call(grid, 0, c.d_boxes, c.n, 8, d_ids) == EINVAL and call(grid, c.d_tris, 0, c.n, 8, d_ids) == EINVAL and call(grid, c.d_tris, c.d_boxes, c.n, 8, 0) == EINVAL
    assert call(grid, c.d_tris + 4, c.d_boxes, c.n, 8, d_ids) == EINVAL
    assert call(grid, c.d_tris, c.d_boxes + 8, c.n - 1, 8, d_ids) == EINVAL
    assert call(grid, c.d_tris, c.d_boxes, c.n, 8, d_ids + 8) == EINVAL and call(grid, c.d_tris, c.d_boxes, c.n, 4, d_ids + 4) == EINVAL
    # 16 bytes only where 16-byte stores are used: any other k writes at any int32 boundary
    mem.one(d_ids, 4 * 8 * c.n + 64)                      # (the k = 8 launch above left its ids here: the ones compared below are this launch's)
    assert call(grid, c.d_tris, c.d_boxes, c.n, 3, d_ids + 4) == 0 and call(grid, c.d_tris, c.d_boxes, c.n, 3, d_ids + 2) == EINVAL
    mem.synchronize()
    assert (mem.download(d_ids + 4, np.int32, 3 * c.n).reshape(c.n, 3) == V.expected(c.fixture, c.name, 3)[0]).all(), "k = 3 at an odd offset"
    assert call(grid, c.d_tris, c.d_boxes, c.n, 8, d_ids, d_cnt + 2) == EINVAL
    assert call(grid, c.d_tris, c.d_boxes, c.n, 8, d_ids, d_cnt, d_tot + 4) == EINVAL
    for flags in (2, 3, 4, 1 << 31):
        assert call(grid, c.d_tris, c.d_boxes, c.n, 1, d_ids, flags=flags) == EINVAL
        assert b"flag" in L.hagrid_last_error(mem._ctx)
        assert lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), 1, d_ids, flags=flags) == EINVAL
    assert call(grid, c.d_tris, c.d_boxes, -1, 8, d_ids) == EINVAL
    assert L.hagrid_overlap_boxes(None, G.pod(grid), vp(c.d_tris), vp(c.d_boxes), c.n, 8, vp(d_ids), None, None, 0) == EINVAL
    # the lattice: n <= 0, too many voxels, a size that is not positive and finite, an origin that is not finite, null arrays
    assert lattice(grid, (0, 0, 0), (1, 1, 1), (4, 4, 2), 1, d_ids, d_cnt) == 0
    G.assert_lattice_refused(lambda origin, size, n: lattice(grid, origin, size, n, 1, d_ids))
    assert lattice(None, (0, 0, 0), (1, 1, 1), (2, 2, 2), 1, d_ids) == EINVAL and lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), 1, 0) == EINVAL
    assert lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), 1, d_ids, tris=0) == EINVAL and lattice(grid, (0, 0, 0), (1, 1, 1), (2, 2, 2), 1, d_ids + 2) == EINVAL
    with pytest.raises(api.HagridError, match="aligned"):
        api.overlap_boxes(grid, c.d_tris, c.d_boxes + 4, 8, 8, d_ids)
    with pytest.raises(api.HagridError, match="voxel"):
        api.voxelize(grid, c.d_tris, (0, 0, 0), (1, 1, 1), (0, 1, 1), 1, d_ids)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.overlap_boxes(g2, c.d_tris, c.d_boxes, c.n, 8, d_ids)
            with pytest.raises(api.HagridError, match="released"):
                api.voxelize(g2, c.d_tris, (0, 0, 0), (1, 1, 1), (2, 2, 2), 1, d_ids)
            assert call(g2, c.d_tris, c.d_boxes, 0, 8, d_ids) == EINVAL
    mem.free(d_ids); mem.free(d_cnt); mem.free(d_tot)
    api.setup_traversal(grid)
    ids, counts = run_overlap(c, grid, c.d_boxes, c.n, 8)
    want_ids, want_counts = V.expected(c.fixture, c.name, 8)
    V.assert_answers_equal(ids, counts, want_ids, want_counts, f"{c.name} after the refused calls")


def test_kernel_budget():
    G.kernel_budget(G.kernel_listing(), one_each=("overlap_boxes_kernel",))         # box-overlap queries are ONE kernel
