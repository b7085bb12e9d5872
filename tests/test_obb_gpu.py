"""Oriented-box queries on the GPU (hagrid_overlap_obbs: obb_tris_kernel of hagrid_amd/csrc/overlap.hip): the device's ids and counts against the fixture
tests/golden/obb.npz on Cell and SmallCell grids built on the device, with a traversal image present and ray binning on, with no image, and with the
nearest-hit hints unmoved around it; ANY, paging and labels; the batch totals against the host walk's; batch sizes at odd offsets; ids at 4-byte alignment;
the deep grids; 100 000 triangles against the host walk over the downloaded grid; torch tensors and the C++ shim; every refusal; the kernel budget.  Every
compared output buffer is poisoned and guarded (tests/_poison.py).  The case and what every query's file checks around its own launches come from
tests/_gpu_case.py."""
import sys

import numpy as np
import pytest

import _deep_grids as D
import _gpu_case as G
import _obb as B
import _overlap as V
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(B.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("obb_host_gpu")
    return B.build_host(d), d


def make_case(name, tris, q, qlab, tlab):
    c = G.open_case(name, tris)
    c.q, c.qlab, c.tlab = q, qlab, tlab
    c.n = q.shape[0]
    c.d_q = c.mem.upload(q)
    c.d_qlab = c.mem.upload(qlab) if qlab is not None else 0
    c.d_tlab = c.mem.upload(tlab) if tlab is not None else 0
    return c


@pytest.fixture(scope="module", params=B.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, records and labels uploaded"""
    tris = B.make_tris(request.param)
    q, qlab = B.scene_queries(fixture, request.param, tris)
    c = make_case(request.param, tris, q, qlab, B.scene_labels(tris.shape[0]))
    c.fixture = fixture
    gb = scene.grid_box(tris)
    for g in c.grids.values():
        assert (g.bbox_min.view(np.uint32) == gb[0].view(np.uint32)).all() and (g.bbox_max.view(np.uint32) == gb[1].view(np.uint32)).all(), "the fixture's grid box"
    yield c
    c.mem.close()


def run_obbs(c, grid, k, flags=0, counts=True, counters=False, labels=True, d_q=None, n=None, offset=0, ids_offset=0):
    """(ids (n, k), counts or None[, the four batch totals]) of queries offset .. offset + n; the outputs are poisoned first and guarded; ids_offset: bytes
    by which the id buffer is moved off its 16-byte alignment"""
    mem = c.mem
    n = c.n if n is None else n
    d_ids = P.alloc_out(mem, 4 * k * n + ids_offset)
    d_cnt = P.alloc_out(mem, 4 * n) if counts else 0
    d_tot = 0
    if counters:
        d_tot = mem.alloc(32); mem.zero(d_tot, 32)
    c.api.overlap_obbs(grid, c.d_tris, (d_q or c.d_q) + 64 * offset, n, k, d_ids + ids_offset, d_cnt, d_tot, flags,
                       query_labels=c.d_qlab + 4 * offset if labels and c.d_qlab else 0, tri_labels=c.d_tlab if labels and c.d_qlab else 0)
    mem.synchronize()
    raw = P.fetch(mem, d_ids, np.uint8, 4 * k * n + ids_offset)
    assert (raw[:ids_offset] == 0xFF).all(), "nothing is written before the ids"
    ids = np.ascontiguousarray(raw[ids_offset:]).view(np.int32).reshape(n, k)
    mem.free(d_ids)
    out = [ids, None]
    if counts:
        out[1] = P.fetch(mem, d_cnt, np.int32, n)
        mem.free(d_cnt)
        P.assert_all_written(out[1])
    if counters:
        out.append(mem.download(d_tot, np.int64, 4))
        mem.free(d_tot)
    return out


def assert_fixture(c, grid, what, ks):
    for k in ks:
        ids, counts = run_obbs(c, grid, k)
        B.assert_answers_equal(ids, counts, *B.expected(c.fixture, c.name + "_lab", k), f"{what} k={k} with labels")


@pytest.mark.parametrize("compress", [False, True])
def test_device_results_equal_the_fixture(case, compress):
    """every query of the fixture with a traversal image present and ray binning on: k = 1, 3, 4, 8 with labels (k = 8: two 16-byte stores per query, k = 4:
    one, the others 4-byte stores), k = 8 without labels, k = 3 without labels and with counts null"""
    c = case
    grid = c.grids[compress]
    what = f"{c.name} compress={compress} image present, binning on"
    with G.image_present(c, grid, binning=True):
        assert_fixture(c, grid, what, (1, 3, 4, 8))
        ids, counts = run_obbs(c, grid, B.KMAX, labels=False)
        B.assert_answers_equal(ids, counts, *B.expected(c.fixture, c.name, B.KMAX), f"{what} k=8 without labels")
        ids, counts = run_obbs(c, grid, 3, labels=False, counts=False)
        assert counts is None
        B.assert_answers_equal(ids, None, B.expected(c.fixture, c.name, 3)[0], None, f"{what} k=3 without labels, counts null")


@pytest.mark.parametrize("compress", [False, True])
def test_no_image_and_the_nearest_hit_hints(case, compress):
    """the same answers (k = 8 and 2) with no traversal image, and between two nearest-hit launches whose hints stay unmoved"""
    c = case
    grid = c.grids[compress]
    G.drop_image(c, grid)
    assert_fixture(c, grid, f"{c.name} compress={compress} no image", (8,))
    with G.nearest_hit_unmoved(c, grid):
        assert_fixture(c, grid, f"{c.name} compress={compress} between two nearest-hit launches", (2,))


@pytest.mark.parametrize("compress", [False, True])
def test_any_paging_and_labels(case, compress):
    """ANY: id >= 0 exactly where |S| > 0, and the id is a member of S (count 0 or 1); labels: no listed triangle of an OWN query belongs to its body;
    paging at k = 3: 64 lists of 4 to 30 members, asked again from first = last id + 1 until they end, are the fixture's lists continued"""
    c = case
    grid = c.grids[compress]
    glo, ghi = scene.grid_box(c.tris)
    boxes = scene.clip_boxes(scene.obb_boxes(c.q, glo, ghi), glo, ghi)
    for key, labels in ((c.name, False), (c.name + "_lab", True)):
        ids, counts = run_obbs(c, grid, 1, flags=c.api.OVERLAP_ANY, labels=labels)
        sizes = c.fixture[key + "_sizes"]
        got = ids[:, 0]
        assert ((got >= 0) == (sizes > 0)).all() and (counts == (sizes > 0)).all() and (got[sizes == 0] == -1).all()
        hit = got >= 0
        assert hit.sum() > 1000
        assert (scene.overlap_pairs(c.tris[got[hit]], boxes[hit]) & scene.obb_pairs(c.tris[got[hit]], c.q[hit])).all() and (got[hit] >= c.q["first"][hit]).all()
        if labels:
            assert not ((c.qlab[hit] >= 0) & (c.tlab[got[hit], 0] == c.qlab[hit])).any()
    ids, _ = run_obbs(c, grid, B.KMAX)
    own = ids[B.OWN]
    assert ((own < 0) | (own // B.BODY != c.qlab[B.OWN, None])).all()
    # paging
    sizes = c.fixture[c.name + "_sizes"][:B.PLANK.start]
    pick = np.flatnonzero((sizes > 3) & (sizes <= 30))[:64]              # at most ten pages each
    assert pick.size == 64
    qq = c.q[pick].copy()
    whole = scene.overlap_obbs(c.tris, qq, k=1 << 12)
    pages = [[] for _ in pick]
    live = np.arange(pick.size)
    for _ in range(int(whole["sizes"].max()) // 3 + 2):
        d_q = c.mem.upload(qq[live])
        ids, counts = run_obbs(c, grid, 3, labels=False, d_q=d_q, n=live.size)
        c.mem.free(d_q)
        for row, i in enumerate(live):
            pages[i] += [int(v) for v in ids[row] if v >= 0]
        more = counts == 4
        qq["first"][live[more]] = ids[more, 2] + 1
        live = live[more]
        if live.size == 0:
            break
    assert live.size == 0
    for i in range(pick.size):
        assert pages[i] == [int(v) for v in whole["ids"][i, :whole["sizes"][i]]], f"query {pick[i]}"


@pytest.mark.parametrize("compress", [False, True])
def test_batch_totals_equal_the_host_walk(case, host, compress):
    c = case
    exe, d = host
    grid = c.grids[compress]
    arrays = grid.download(c.mem)
    for k, flags, labels in ((8, 0, True), (1, 0, False), (1, c.api.OVERLAP_ANY, True)):
        ids, counts, tot = run_obbs(c, grid, k, flags=flags, counters=True, labels=labels)
        w_ids, w_counts, totals = B.host_walk(exe, d, arrays, c.tris, c.q, k, c.qlab if labels else None, c.tlab if labels else None, any_=bool(flags))
        B.assert_answers_equal(ids, counts, w_ids, w_counts, f"{c.name} compress={compress} k={k} flags={flags} against the host walk over the device's grid")
        assert tot.tolist() == [c.n, int(totals[:, 0].astype(np.int64).sum()), int(totals[:, 1].astype(np.int64).sum()), int(totals[:, 2].astype(np.int64).sum())]
        assert tot[1] > 0 and tot[2] > 0 and tot[3] > 0
    d_ids = c.mem.alloc(4 * c.n)
    G.assert_totals_added(lambda d_tot: c.api.overlap_obbs(grid, c.d_tris, c.d_q, c.n, 1, d_ids, 0, d_tot, c.api.OVERLAP_ANY, query_labels=c.d_qlab, tri_labels=c.d_tlab),
                          c.mem, tot)
    c.mem.free(d_ids)


def test_batch_shapes_and_alignment(case):
    """batches of 1, 63, 64, 65 and 4095 queries at odd offsets into the record buffer: the tail of a wavefront writes nothing -- the guard behind n * k ids
    and n counts stays untouched; k = 4 and 8 with aligned ids, the other k with ids at a 4-byte boundary that is no 16-byte boundary"""
    c = case
    grid = c.grids[True]
    c.api.overlap_obbs(grid, c.d_tris, 0, 0, 3, 0)                 # no queries: nothing is launched, null buffers are fine
    c.api.overlap_obbs(grid, 0, 0, 0, 8, 0, 0, 0)
    for n, offset in ((1, 3), (63, 5), (64, B.PLANK.start - 31), (65, B.BAD.start - 21), (4095, 1)):
        for k, ids_offset in ((3, 4), (4, 0), (8, 0), (5, 12)) if n < 4095 else ((8, 0), (2, 4)):
            ids, counts = run_obbs(c, grid, k, n=n, offset=offset, ids_offset=ids_offset)
            want_ids, want_counts = B.expected(c.fixture, c.name + "_lab", k)
            B.assert_answers_equal(ids, counts, want_ids[offset:offset + n], want_counts[offset:offset + n], f"{c.name} n={n} offset={offset} k={k}")


@pytest.mark.parametrize("name", D.WALKED)
def test_deep_grids(host, name):
    """the deep grids of tests/_deep_grids.py, finished on the device: rotated boxes and planks against the host walk over the downloaded grid and the
    brute force"""
    from hagrid_amd import api
    exe, d = host
    tris = D.make_tris(name)
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    cen = np.concatenate([V.vertices_of(tris[1500 if name == "nested" else 0:], 192, B.SEED + 50), scene.make_points_uniform(lo, hi, 64, B.SEED + 51)])
    half = (np.float32([1e-5, 1e-4, 1e-3, 5e-2])[np.arange(256) % 4][:, None] * (np.float32(0.5) + B._u(B.SEED + 52, 256, 3)) * diag).astype(np.float32)
    q = np.concatenate([B._rotated(cen, B.rotations(B.SEED + 53, 256), half), B.plank_records(lo, hi, 16, B.SEED + 54)])
    c = G.upload_case(tris, name)
    c.q, c.n, c.d_q, c.d_qlab, c.d_tlab = q, q.shape[0], c.mem.upload(q), 0, 0
    st = D.DeviceStages(name, api, c.mem, c.d_tris, tris.shape[0])
    for stage in D.stages_of(name):
        out = D.stage_grid(st, stage)
        grid = st.grid
        arrays = grid.download(c.mem)
        for k in (1, 8):
            ids, counts, tot = run_obbs(c, grid, k, counters=True, labels=False)
            w_ids, w_counts, totals = B.host_walk(exe, d, arrays, tris, q, k)
            B.assert_answers_equal(ids, counts, w_ids, w_counts, f"{name} {stage} k={k} against the host walk")
            assert tot[1:].tolist() == [int(totals[:, j].astype(np.int64).sum()) for j in range(3)]
            B.assert_answers_equal(ids, counts, *B.host_brute(exe, d, tris, q, k, grid=(grid.bbox_min, grid.bbox_max)), f"{name} {stage} k={k} against the brute force")
    st.grid.free()
    c.mem.close()


def test_hundred_thousand_triangles_against_the_host_walk(host):
    exe, d = host
    tris = scene.make_soup(100000)
    lo, hi = scene.tris_bbox(tris)
    diag = scene.bbox_diagonal(lo, hi)
    n = 2048
    half = ((np.float32(0.002) + np.float32(0.02) * B._u(B.SEED + 60, n, 3)) * diag).astype(np.float32)
    q = np.concatenate([B._rotated(scene.make_points_near_surface(tris, lo, hi, n, B.SEED + 61), B.rotations(B.SEED + 62, n), half), B.plank_records(lo, hi, 64, B.SEED + 63)])
    c = make_case("soup100k", tris, q, None, None)
    for compress in (False, True):
        grid = c.grids[compress]
        arrays = grid.download(c.mem)
        ids, counts, tot = run_obbs(c, grid, B.KMAX, counters=True)
        w_ids, w_counts, totals = B.host_walk(exe, d, arrays, tris, q, B.KMAX)
        B.assert_answers_equal(ids, counts, w_ids, w_counts, f"100 000 triangles compress={compress}")
        assert tot[1:].tolist() == [int(totals[:, j].astype(np.int64).sum()) for j in range(3)] and (counts > 0).sum() > n // 2
    c.mem.close()


def test_torch_records_and_paged_lists():
    """api.obb_records and api.tris_in_obbs on a torch stream: a rigid body's box against the scene, two frames; every list is scene.overlap_obbs's whole set"""
    import torch
    from hagrid_amd import api
    tris = B.make_tris("mesh")
    nt = tris.shape[0]
    lo, hi = scene.tris_bbox(tris)
    diag = float(scene.bbox_diagonal(lo, hi))
    mem = api.MemManager(keep=True)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            t_tris = torch.from_numpy(tris).cuda()
            grid = api.build_all(mem, t_tris.data_ptr(), nt)
            n = 96
            R = torch.from_numpy(B.rotations(B.SEED + 70, n)).cuda()
            half = torch.from_numpy(((np.float32(0.01) + np.float32(0.04) * B._u(B.SEED + 71, n, 3)) * np.float32(diag)).astype(np.float32)).cuda()
            lab = torch.arange(n, dtype=torch.int32, device="cuda") % 8
            t_lab = torch.from_numpy(B.scene_labels(nt)).cuda()
            for frame in range(2):
                cen = torch.from_numpy(scene.make_points_near_surface(tris, lo, hi, n, B.SEED + 72 + frame)).cuda()
                rec = api.obb_records(cen, R, half)
                assert rec.shape == (n, 16) and rec.dtype == torch.float32 and rec.is_cuda
                want_rec = B._rotated(cen.cpu().numpy(), R.cpu().numpy(), half.cpu().numpy())
                assert (rec.cpu().numpy().view(np.uint32) == scene._obb_rows(want_rec).view(np.uint32)).all(), "obb_records makes scene.make_obbs's records"
                got = api.tris_in_obbs(grid, t_tris, rec, k=4, query_labels=lab, tri_labels=t_lab)
                want = scene.overlap_obbs(tris, want_rec, k=1 << 12, query_labels=lab.cpu().numpy(), tri_labels=t_lab.cpu().numpy(), grid=(grid.bbox_min, grid.bbox_max))
                off = got["offsets"].cpu().numpy(); ids = got["ids"].cpu().numpy()
                assert got["complete"] and got["pages"] > 2 and (np.diff(off) == want["sizes"]).all() and off[-1] > 4 * n
                for i in range(n):
                    assert (ids[off[i]:off[i + 1]] == want["ids"][i, :want["sizes"][i]]).all(), f"frame {frame} box {i}"
            part = api.tris_in_obbs(grid, t_tris, rec, k=4, max_pages=1)
            assert not part["complete"] and part["pages"] == 1
            grid.free()
            stream.synchronize()
    finally:
        mem.use_stream(None)
    mem.close()


def test_cpp_program_through_the_shim(tmp_path):
    import _subproc
    r = _subproc.check([G.build_shim("obb", tmp_path), "20000", "1000"], timeout=120)
    sys.stdout.write(r.stdout)
    assert " 0 mismatches vs host brute force" in r.stdout, r.stdout


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

    def call(g, tris, obbs, n, k, ids, counts=0, counters=0, flags=0, qlab=0, tlab=0):
        return L.hagrid_overlap_obbs(mem._ctx, G.pod(g), vp(tris), vp(obbs), n, vp(qlab), vp(tlab), k, vp(ids), vp(counts), vp(counters), flags)

    assert call(grid, c.d_tris, c.d_q, c.n, 8, d_ids, d_cnt, d_tot, qlab=c.d_qlab, tlab=c.d_tlab) == 0
    assert call(None, c.d_tris, c.d_q, c.n, 8, d_ids) == EINVAL and b"grid" in L.hagrid_last_error(mem._ctx)
    for k in (0, -1, 9, 1 << 20):
        assert call(grid, c.d_tris, c.d_q, c.n, k, d_ids) == EINVAL and b"k must" in L.hagrid_last_error(mem._ctx)
    for k in (2, 8):
        assert call(grid, c.d_tris, c.d_q, c.n, k, d_ids, flags=ANY) == EINVAL and b"k = 1" in L.hagrid_last_error(mem._ctx)
    assert call(grid, 0, c.d_q, c.n, 8, d_ids) == EINVAL and call(grid, c.d_tris, 0, c.n, 8, d_ids) == EINVAL and call(grid, c.d_tris, c.d_q, c.n, 8, 0) == EINVAL
    assert call(grid, c.d_tris + 4, c.d_q, c.n, 8, d_ids) == EINVAL
    assert call(grid, c.d_tris, c.d_q + 8, c.n - 1, 8, d_ids) == EINVAL and b"aligned" in L.hagrid_last_error(mem._ctx)
    assert call(grid, c.d_tris, c.d_q, c.n, 8, d_ids + 8) == EINVAL and call(grid, c.d_tris, c.d_q, c.n, 4, d_ids + 4) == EINVAL
    assert call(grid, c.d_tris, c.d_q, c.n, 3, d_ids + 2) == EINVAL
    assert call(grid, c.d_tris, c.d_q, c.n, 8, d_ids, d_cnt + 2) == EINVAL
    assert call(grid, c.d_tris, c.d_q, c.n, 8, d_ids, d_cnt, d_tot + 4) == EINVAL
    # one label array without the other; misaligned labels
    assert call(grid, c.d_tris, c.d_q, c.n, 8, d_ids, qlab=c.d_qlab) == EINVAL and b"together" in L.hagrid_last_error(mem._ctx)
    assert call(grid, c.d_tris, c.d_q, c.n, 8, d_ids, tlab=c.d_tlab) == EINVAL
    assert call(grid, c.d_tris, c.d_q, c.n, 8, d_ids, qlab=c.d_qlab + 2, tlab=c.d_tlab) == EINVAL
    assert call(grid, c.d_tris, c.d_q, c.n, 8, d_ids, qlab=c.d_qlab, tlab=c.d_tlab + 1) == EINVAL
    assert call(grid, c.d_tris, c.d_q, 0, 8, 0, qlab=c.d_qlab) == EINVAL, "checked before the empty batch returns"
    for flags in (2, 3, 4, 1 << 31):
        assert call(grid, c.d_tris, c.d_q, c.n, 1, d_ids, flags=flags) == EINVAL and b"flag" in L.hagrid_last_error(mem._ctx)
    assert call(grid, c.d_tris, c.d_q, -1, 8, d_ids) == EINVAL
    assert call(grid, 0, 0, 0, 8, 0) == 0, "num_obbs = 0 is fine with null buffers"
    assert L.hagrid_overlap_obbs(None, G.pod(grid), vp(c.d_tris), vp(c.d_q), c.n, None, None, 8, vp(d_ids), None, None, 0) == EINVAL
    with pytest.raises(api.HagridError, match="aligned"):
        api.overlap_obbs(grid, c.d_tris, c.d_q + 4, 8, 8, d_ids)
    with pytest.raises(api.HagridError, match="together"):
        api.overlap_obbs(grid, c.d_tris, c.d_q, 8, 8, d_ids, tri_labels=c.d_tlab)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.overlap_obbs(g2, c.d_tris, c.d_q, c.n, 8, d_ids)
    mem.free(d_ids); mem.free(d_cnt); mem.free(d_tot)
    # the context still works: the next box query equals its fixture, and so does the next oriented-box query
    box_fixture = np.load(V.FIXTURE)
    boxes = V.scene_boxes(box_fixture, c.name, c.tris)
    d_boxes = mem.upload(boxes)
    d_out = P.alloc_out(mem, 4 * 8 * boxes.shape[0]); d_oc = P.alloc_out(mem, 4 * boxes.shape[0])
    api.overlap_boxes(grid, c.d_tris, d_boxes, boxes.shape[0], 8, d_out, d_oc)
    mem.synchronize()
    V.assert_answers_equal(P.fetch(mem, d_out, np.int32, 8 * boxes.shape[0]).reshape(-1, 8), P.fetch(mem, d_oc, np.int32, boxes.shape[0]), *V.expected(box_fixture, c.name, 8),
                           f"{c.name}: boxes after the refused calls")
    mem.free(d_boxes); mem.free(d_out); mem.free(d_oc)
    ids, counts = run_obbs(c, grid, 8)
    B.assert_answers_equal(ids, counts, *B.expected(c.fixture, c.name + "_lab", 8), f"{c.name} after the refused calls")


def test_kernel_budget():
    G.kernel_budget(G.kernel_listing(), one_each=("obb_tris_kernel", "overlap_boxes_kernel"))
