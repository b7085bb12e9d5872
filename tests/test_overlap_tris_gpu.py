"""Contact queries on the GPU (hagrid_overlap_tris: the contact mode of the kernel of hagrid_amd/csrc/overlap.hip): the device's ids and counts against the
fixture tests/golden/overlap_tris.npz -- the queries of two scenes and a lattice scene whose truth is exact arithmetic -- on Cell and SmallCell grids built
on the device, for k = 1, 2, 3, 4, 5, 8, with counts, first and labels given and null; ANY; the batch totals against the host walk's; batch tails; the scene's
own array as queries; the frame loop of two MeshScenes from torch tensors; a C++ program through the shim; every argument error; the kernel budget.  Every
compared output buffer is poisoned and guarded (tests/_poison.py).
The case and what every query's file checks around its own launches come from tests/_gpu_case.py."""
import sys

import numpy as np
import pytest

import _gpu_case as G
import _overlap as V
import _overlap_tris as W
import _poison as P
from hagrid_amd import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(W.FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_tris_host_gpu")
    return W.build_host(d), d


def make_case(name, tris, queries, first, qlab, tlab):
    c = G.open_case(name, tris)
    c.queries, c.first, c.qlab, c.tlab = queries, first, qlab, tlab
    c.n = queries.shape[0]
    c.d_queries = c.mem.upload(queries)
    c.d_first = c.mem.upload(first) if first is not None else 0
    c.d_qlab = c.mem.upload(qlab) if qlab is not None else 0
    c.d_tlab = c.mem.upload(tlab) if tlab is not None else 0
    return c


@pytest.fixture(scope="module", params=W.SCENES)
def case(request, fixture):
    """one scene of the fixture: Cell and SmallCell grids built on the device, queries, firsts and labels uploaded"""
    tris = W.make_tris(request.param)
    q, first, qlab = W.scene_queries(fixture, request.param, tris)
    c = make_case(request.param, tris, q, first, qlab, W.scene_labels(request.param, tris.shape[0]))
    c.fixture = fixture
    gb = scene.grid_box(tris)
    for g in c.grids.values():
        assert (g.bbox_min.view(np.uint32) == gb[0].view(np.uint32)).all() and (g.bbox_max.view(np.uint32) == gb[1].view(np.uint32)).all(), "the fixture's grid box"
    yield c
    c.mem.close()


@pytest.fixture(scope="module")
def lattice_case(fixture):
    tris, queries, _, _ = W.lattice_scene()
    assert W.array_sum(tris) + W.array_sum(queries) == int(fixture["lattice_scene_sum"])
    c = make_case("lattice", tris, queries, None, None, None)
    c.fixture = fixture
    yield c
    c.mem.close()


def run_tris(c, grid, k, flags=0, counts=True, counters=False, first=True, labels=True, d_queries=None, n=None, offset=0):
    """(ids (n, k), counts or None[, the four batch totals]) of queries offset .. offset + n; the outputs are poisoned first and guarded"""
    mem = c.mem
    n = c.n if n is None else n
    d_ids = P.alloc_out(mem, 4 * k * n)
    d_cnt = P.alloc_out(mem, 4 * n) if counts else 0
    d_tot = 0
    if counters:
        d_tot = mem.alloc(32); mem.zero(d_tot, 32)
    c.api.overlap_tris(grid, c.d_tris, (d_queries or c.d_queries) + 48 * offset, n, k, d_ids, d_cnt, d_tot, flags,
                       first=c.d_first + 4 * offset if first and c.d_first else 0,
                       query_labels=c.d_qlab + 12 * offset if labels and c.d_qlab else 0, tri_labels=c.d_tlab if labels and c.d_qlab else 0)
    mem.synchronize()
    ids = P.fetch(mem, d_ids, np.int32, k * n).reshape(n, k)
    mem.free(d_ids)
    out = [ids, None]                                     # (an untouched id reads -1, an empty slot: only the comparison with the expected ids tells; an untouched count tells by itself)
    if counts:
        out[1] = P.fetch(mem, d_cnt, np.int32, n)
        mem.free(d_cnt)
        P.assert_all_written(out[1])
    if counters:
        out.append(mem.download(d_tot, np.int64, 4))
        mem.free(d_tot)
    return out


@pytest.mark.parametrize("compress", [False, True])
def test_device_results_equal_the_fixture(case, compress):
    """every query of (c), k = 1, 2, 3, 4, 5, 8 (k = 8: two 16-byte stores per query, k = 4: one, the others 4-byte stores), with first and labels; with
    first alone; with neither; counts null"""
    c = case
    grid = c.grids[compress]
    for k in W.KS:
        ids, counts = run_tris(c, grid, k)
        W.assert_answers_equal(ids, counts, *W.expected(c.fixture, c.name + "_lab", k), f"{c.name} compress={compress} k={k} with first and labels")
        if k in (2, 8):
            ids, counts = run_tris(c, grid, k, labels=False)
            W.assert_answers_equal(ids, counts, *W.expected(c.fixture, c.name, k), f"{c.name} compress={compress} k={k} with first")
    for k in (8, 3):
        ids, counts = run_tris(c, grid, k, first=False, labels=False, counts=False)
        assert counts is None
        W.assert_answers_equal(ids, None, W.expected(c.fixture, c.name, k, first=False)[0], None, f"{c.name} compress={compress} k={k} with neither, counts null")


@pytest.mark.parametrize("compress", [False, True])
def test_lattice_scene_equals_the_exact_test(lattice_case, compress):
    """(d): the device's answers are the exact test's"""
    c = lattice_case
    for k in W.KS:
        ids, counts = run_tris(c, c.grids[compress], k)
        W.assert_answers_equal(ids, counts, *W.expected(c.fixture, "lattice", k), f"lattice scene compress={compress} k={k}")
    ids, counts = run_tris(c, c.grids[compress], 1, flags=c.api.OVERLAP_ANY)
    sizes = c.fixture["lattice_sizes"]
    assert ((ids[:, 0] >= 0) == (sizes > 0)).all() and (counts == (sizes > 0)).all()


@pytest.mark.parametrize("compress", [False, True])
def test_any(case, compress):
    """id >= 0 exactly where |S| > 0, and the returned id is a member of S: it meets the query's box and the query, respects first and shares no label"""
    c = case
    glo, ghi = scene.grid_box(c.tris)
    boxes = scene.clip_boxes(scene.query_boxes(c.queries, glo, ghi), glo, ghi)
    for key, labels in ((c.name, False), (c.name + "_lab", True)):
        ids, counts = run_tris(c, c.grids[compress], 1, flags=c.api.OVERLAP_ANY, labels=labels)
        sizes = c.fixture[key + "_sizes"]
        got = ids[:, 0]
        assert ((got >= 0) == (sizes > 0)).all() and (counts == (sizes > 0)).all() and (got[sizes == 0] == -1).all()
        hit = got >= 0
        assert hit.sum() > 1000
        assert (scene.overlap_pairs(c.tris[got[hit]], boxes[hit]) & scene.tri_tri_pairs(c.queries[hit], c.tris[got[hit]])).all() and (got[hit] >= c.first[hit]).all()
        if labels:
            assert not scene.labels_shared(c.qlab[hit], c.tlab[got[hit]]).any()


@pytest.mark.parametrize("compress", [False, True])
def test_batch_totals_equal_the_host_walk(case, host, compress):
    c = case
    exe, d = host
    grid = c.grids[compress]
    arrays = grid.download(c.mem)
    for k, flags, labels in ((8, 0, True), (1, 0, False), (1, c.api.OVERLAP_ANY, True)):
        ids, counts, tot = run_tris(c, grid, k, flags=flags, counters=True, labels=labels)
        w_ids, w_counts, totals = W.host_walk(exe, d, arrays, c.tris, c.queries, k, c.first, c.qlab if labels else None, c.tlab if labels else None, any_=bool(flags))
        W.assert_answers_equal(ids, counts, w_ids, w_counts, f"{c.name} compress={compress} k={k} flags={flags} against the host walk over the device's grid")
        assert tot.tolist() == [c.n, int(totals[:, 0].astype(np.int64).sum()), int(totals[:, 1].astype(np.int64).sum()), int(totals[:, 2].astype(np.int64).sum())]
        assert tot[1] > 0 and tot[2] > 0 and tot[3] > 0
    # the totals are ADDED: a second launch doubles them
    d_ids = c.mem.alloc(4 * c.n)
    G.assert_totals_added(lambda d_tot: c.api.overlap_tris(grid, c.d_tris, c.d_queries, c.n, 1, d_ids, 0, d_tot, c.api.OVERLAP_ANY, first=c.d_first, query_labels=c.d_qlab,
                                                           tri_labels=c.d_tlab), c.mem, tot)
    c.mem.free(d_ids)


def test_batch_tails(case):
    """batches of 1, 63, 64, 65 and 129 queries, at an offset into the query buffer (the huge queries among them): the tail of a wavefront writes nothing --
    the guard behind n * k ids and n counts stays untouched"""
    c = case
    grid = c.grids[True]
    c.api.overlap_tris(grid, c.d_tris, 0, 0, 3, 0)                 # no queries: nothing is launched, null buffers are fine
    c.api.overlap_tris(grid, 0, 0, 0, 8, 0, 0, 0)
    for n, offset in ((1, 0), (63, 5), (64, W.HUGE.start - 30), (65, W.INACTIVE.start - 20), (129, W.NUM_QUERIES - 129)):
        for k in (3, 4, 8):
            ids, counts = run_tris(c, grid, k, n=n, offset=offset)
            want_ids, want_counts = W.expected(c.fixture, c.name + "_lab", k)
            W.assert_answers_equal(ids, counts, want_ids[offset:offset + n], want_counts[offset:offset + n], f"{c.name} n={n} offset={offset} k={k}")


def test_queries_may_be_the_scene(case):
    """queries == tris: the first 4096 triangles of the scene ask over their own array, with their labels and first[i] = i + 1 -- every pair once"""
    c = case; mem = c.mem
    n = min(c.tris.shape[0], 4096)
    first = np.arange(1, n + 1, dtype=np.int32)
    want = scene.overlap_tris(c.tris, c.tris[:n], k=5, first=first, query_labels=c.tlab[:n], tri_labels=c.tlab)
    d_first = mem.upload(first)
    d_ids = P.alloc_out(mem, 4 * 5 * n); d_cnt = P.alloc_out(mem, 4 * n)
    c.api.overlap_tris(c.grids[False], c.d_tris, c.d_tris, n, 5, d_ids, d_cnt, first=d_first, query_labels=c.d_tlab, tri_labels=c.d_tlab)
    mem.synchronize()
    ids = P.fetch(mem, d_ids, np.int32, 5 * n).reshape(n, 5); counts = P.fetch(mem, d_cnt, np.int32, n)
    W.assert_answers_equal(ids, counts, want["ids"], want["counts"], f"{c.name}: the scene against itself")
    assert (ids[ids >= 0] > np.repeat(np.arange(n), 5)[ids.reshape(-1) >= 0]).all() and (counts > 0).sum() > 30
    mem.free(d_ids); mem.free(d_cnt); mem.free(d_first)


def test_frame_loop_from_torch_tensors():
    """two MeshScenes on torch's stream, one moved by a transform per frame: assemble both -> build the grid of the first -> the contacts of the second
    against it, with every buffer a torch tensor; then the self-intersections of the first with its vertex labels.  Every answer is scene.overlap_tris's
    on the triangles of that frame."""
    import torch
    from hagrid_amd import api
    verts, faces, solids = scene.make_stadium_mesh(0.05, solids_only=True)
    verts = np.ascontiguousarray(verts, np.float32); faces = np.ascontiguousarray(faces, np.int32)
    f0, nf = solids[0]["faces"]                                     # the moving body: the first torus, as a mesh of its own
    body = np.ascontiguousarray(faces[f0:f0 + nf])
    nt = faces.shape[0]
    mem = api.MemManager(keep=True)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            mem.use_stream(torch.cuda.current_stream().cuda_stream)
            tV = torch.from_numpy(verts).cuda(); tF = torch.from_numpy(faces).cuda(); tB = torch.from_numpy(body).cuda()
            fixed = api.MeshScene(mem, [(tV.data_ptr(), verts.shape[0], tF.data_ptr(), nt)])
            moving = api.MeshScene(mem, [(tV.data_ptr(), verts.shape[0], tB.data_ptr(), nf)], instance_mesh=[0, 0])
            t_tris = torch.zeros((nt, 12), dtype=torch.float32, device="cuda")
            t_q = torch.zeros((2 * nf, 12), dtype=torch.float32, device="cuda")
            fixed.assemble(0, t_tris.data_ptr())
            grid = api.build_all(mem, t_tris.data_ptr(), nt)
            tris = t_tris.cpu().numpy()
            labels = fixed.vertex_labels()
            assert labels.dtype == torch.int32 and labels.is_cuda and (labels.cpu().numpy() == faces).all()
            ml = moving.vertex_labels().cpu().numpy()
            assert (ml[:nf] == body).all() and (ml[nf:] == body + verts.shape[0]).all(), "instances never share a label"
            for frame in range(2):
                M = np.array([[1, 0, 0, 0.02 + 0.05 * frame, 0, 1, 0, 0.01, 0, 0, 1, -0.03 * frame],
                              [0, 0, 1, 0.1, 0, 1, 0, 0.02 * frame, -1, 0, 0, 0.7]], dtype=np.float32)
                tM = torch.from_numpy(M).cuda()
                moving.assemble(tM.data_ptr(), t_q.data_ptr())
                t_ids = torch.full((2 * nf, 4), -7, dtype=torch.int32, device="cuda")
                t_cnt = torch.full((2 * nf,), -7, dtype=torch.int32, device="cuda")
                t_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
                api.overlap_tris(grid, t_tris.data_ptr(), t_q.data_ptr(), 2 * nf, 4, t_ids.data_ptr(), t_cnt.data_ptr(), t_tot.data_ptr())
                touching = (t_cnt > 0).sum()                          # torch work on the same stream, after the launch
                q = t_q.cpu().numpy()
                assert (q.view(np.uint32) == scene.assemble_tris([(verts, body)], [0, 0], M)[0].view(np.uint32)).all()
                want = scene.overlap_tris(tris, q, k=4, grid=(grid.bbox_min, grid.bbox_max))
                W.assert_answers_equal(t_ids.cpu().numpy(), t_cnt.cpu().numpy(), want["ids"], want["counts"], f"frame {frame}")
                assert int(touching) == int((want["sizes"] > 0).sum()) > 20 and int(t_tot[0]) == 2 * nf and int(t_tot[2]) > 0
            ids, counts = api.self_intersections(grid, t_tris, labels, 8)
            want = scene.overlap_tris(tris, tris, k=8, first=np.arange(1, nt + 1), query_labels=faces, tri_labels=faces, grid=(grid.bbox_min, grid.bbox_max))
            W.assert_answers_equal(ids.cpu().numpy(), counts.cpu().numpy(), want["ids"], want["counts"], "self-intersections")
            assert (want["sizes"] == 0).all() and (counts == 0).all(), "the closed solids of the stadium are clean: no triangle touches one that is no neighbour"
            grid.free()
            stream.synchronize()
            fixed.close(); moving.close()
    finally:
        mem.use_stream(None)
    mem.close()


def test_cpp_program_through_the_shim(tmp_path):
    import _subproc
    r = _subproc.check([G.build_shim("overlap_tris", tmp_path), "20000", "1000"], timeout=120)
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

    def call(g, tris, queries, n, k, ids, counts=0, counters=0, flags=0, first=0, qlab=0, tlab=0):
        return L.hagrid_overlap_tris(mem._ctx, G.pod(g), vp(tris), vp(queries), n, vp(first), vp(qlab), vp(tlab), k, vp(ids), vp(counts), vp(counters), flags)

    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids, d_cnt, d_tot, first=c.d_first, qlab=c.d_qlab, tlab=c.d_tlab) == 0
    assert call(None, c.d_tris, c.d_queries, c.n, 8, d_ids) == EINVAL and b"grid" in L.hagrid_last_error(mem._ctx)
    for k in (0, -1, 9, 1 << 20):
        assert call(grid, c.d_tris, c.d_queries, c.n, k, d_ids) == EINVAL and b"k must" in L.hagrid_last_error(mem._ctx)
    for k in (2, 8):
        assert call(grid, c.d_tris, c.d_queries, c.n, k, d_ids, flags=ANY) == EINVAL and b"k = 1" in L.hagrid_last_error(mem._ctx)
    assert call(grid, 0, c.d_queries, c.n, 8, d_ids) == EINVAL and call(grid, c.d_tris, 0, c.n, 8, d_ids) == EINVAL and call(grid, c.d_tris, c.d_queries, c.n, 8, 0) == EINVAL
    assert call(grid, c.d_tris + 4, c.d_queries, c.n, 8, d_ids) == EINVAL
    assert call(grid, c.d_tris, c.d_queries + 8, c.n - 1, 8, d_ids) == EINVAL and b"aligned" in L.hagrid_last_error(mem._ctx)
    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids + 8) == EINVAL and call(grid, c.d_tris, c.d_queries, c.n, 4, d_ids + 4) == EINVAL
    assert call(grid, c.d_tris, c.d_queries, c.n, 3, d_ids + 2) == EINVAL
    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids, d_cnt + 2) == EINVAL
    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids, d_cnt, d_tot + 4) == EINVAL
    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids, first=c.d_first + 2) == EINVAL
    # one label array without the other; misaligned labels
    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids, qlab=c.d_qlab) == EINVAL and b"together" in L.hagrid_last_error(mem._ctx)
    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids, tlab=c.d_tlab) == EINVAL
    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids, qlab=c.d_qlab + 2, tlab=c.d_tlab) == EINVAL
    assert call(grid, c.d_tris, c.d_queries, c.n, 8, d_ids, qlab=c.d_qlab, tlab=c.d_tlab + 1) == EINVAL
    assert call(grid, c.d_tris, c.d_queries, 0, 8, 0, qlab=c.d_qlab) == EINVAL, "checked before the empty batch returns"
    for flags in (2, 3, 4, 1 << 31):
        assert call(grid, c.d_tris, c.d_queries, c.n, 1, d_ids, flags=flags) == EINVAL and b"flag" in L.hagrid_last_error(mem._ctx)
    assert call(grid, c.d_tris, c.d_queries, -1, 8, d_ids) == EINVAL
    assert call(grid, 0, 0, 0, 8, 0) == 0, "num_queries = 0 is fine with null buffers"
    assert L.hagrid_overlap_tris(None, G.pod(grid), vp(c.d_tris), vp(c.d_queries), c.n, None, None, None, 8, vp(d_ids), None, None, 0) == EINVAL
    # 16 bytes only where 16-byte stores are used: any other k writes at any int32 boundary
    mem.one(d_ids, 4 * 8 * c.n + 64)
    assert call(grid, c.d_tris, c.d_queries, c.n, 3, d_ids + 4, first=c.d_first) == 0
    mem.synchronize()
    assert (mem.download(d_ids + 4, np.int32, 3 * c.n).reshape(c.n, 3) == W.expected(c.fixture, c.name, 3)[0]).all(), "k = 3 at an odd offset"
    with pytest.raises(api.HagridError, match="aligned"):
        api.overlap_tris(grid, c.d_tris, c.d_queries + 4, 8, 8, d_ids)
    with pytest.raises(api.HagridError, match="together"):
        api.overlap_tris(grid, c.d_tris, c.d_queries, 8, 8, d_ids, tri_labels=c.d_tlab)
    # a grid given up for traversal has no construction format left
    with G.released_grid(c) as g2:
        if g2 is not None:
            with pytest.raises(api.HagridError, match="released"):
                api.overlap_tris(g2, c.d_tris, c.d_queries, c.n, 8, d_ids)
    mem.free(d_ids); mem.free(d_cnt); mem.free(d_tot)
    # the context still works: the next box query equals its fixture, and so does the next contact query
    box_fixture = np.load(V.FIXTURE)
    boxes = V.scene_boxes(box_fixture, c.name, c.tris)
    d_boxes = mem.upload(boxes)
    d_out = P.alloc_out(mem, 4 * 8 * boxes.shape[0]); d_oc = P.alloc_out(mem, 4 * boxes.shape[0])
    api.overlap_boxes(grid, c.d_tris, d_boxes, boxes.shape[0], 8, d_out, d_oc)
    mem.synchronize()
    V.assert_answers_equal(P.fetch(mem, d_out, np.int32, 8 * boxes.shape[0]).reshape(-1, 8), P.fetch(mem, d_oc, np.int32, boxes.shape[0]), *V.expected(box_fixture, c.name, 8),
                           f"{c.name}: boxes after the refused calls")
    mem.free(d_boxes); mem.free(d_out); mem.free(d_oc)
    ids, counts = run_tris(c, grid, 8)
    W.assert_answers_equal(ids, counts, *W.expected(c.fixture, c.name + "_lab", 8), f"{c.name} after the refused calls")


def test_kernel_budget():
    G.kernel_budget(G.kernel_listing(), one_each=("overlap_boxes_kernel",), absent=("overlap_tris_kernel",))     # contact queries are a mode of the ONE box-overlap kernel
