"""Scenes assembled on the device (hagrid_amd/csrc/assemble.hip) on the GPU: hagrid_scene_assemble against the numpy statement
scene.assemble_tris byte for byte -- meshes, indices and matrices as torch tensors --, the stadium mesh through assemble -> build -> traversal
against the CPU oracle, a frame loop on one stream whose matrices torch computes on the device, the front-end's --device-tris, and every
argument error.  Every comparison of triangles is of all 48 bytes of every triangle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _assemble_scene as S
import _subproc
from _poison import alloc_out, fetch
from hagrid_amd import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_tris(got, want):
    return got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes()


def to_device(meshes):
    """the meshes as torch tensors on the device: ([(vertices, faces | None)], [MeshScene records])"""
    import torch
    tensors, recs = [], []
    for v, f, nf in meshes:
        tv = torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
        tf = torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda() if f is not None and nf else None
        tensors.append((tv, tf))
        recs.append((tv.data_ptr(), v.shape[0], tf.data_ptr() if tf is not None else 0, nf, 4 * v.shape[1]))
    torch.cuda.synchronize()
    return tensors, recs


def statement(meshes, instance_mesh, transforms):
    return scene.assemble_tris([(v, f) if f is not None else (v, None, n) for v, f, n in meshes], instance_mesh, transforms)


@pytest.fixture(scope="module")
def mem():
    from hagrid_amd import api
    m = api.MemManager(keep=True)
    yield m
    m.close()


def test_shared_scene_equals_the_statement_and_follows_rewritten_vertices(mem):
    import torch
    from hagrid_amd import api
    meshes = S.make_meshes()
    tensors, recs = to_device(meshes)
    ms = api.MeshScene(mem, recs, S.INSTANCE_MESH)
    sizes = [meshes[k][2] for k in S.INSTANCE_MESH]
    n = sum(sizes)
    assert ms.num_tris == n and ms.num_instances == len(sizes)
    assert [ms.first_tri(i) for i in range(len(sizes) + 1)] == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    d_tris = mem.alloc(48 * n + 48); d_org = mem.alloc(8 * n + 8)

    def run(transforms, meshes_now, with_origins=True):
        t = torch.from_numpy(transforms).cuda() if transforms is not None else None
        torch.cuda.synchronize()
        mem.one(d_tris, 48 * n + 48); mem.one(d_org, 8 * n + 8)
        ms.assemble(t.data_ptr() if t is not None else 0, d_tris, d_org if with_origins else 0)
        got = mem.download(d_tris, np.float32, 12 * n + 12)
        org = mem.download(d_org, np.int32, 2 * n + 2)
        want, want_org, want_bad = statement(meshes_now, S.INSTANCE_MESH, transforms)
        diff = (bits(got[:12 * n].reshape(n, 12)) != bits(want)).any(axis=1)
        assert not diff.any(), f"{diff.sum()} of {n} triangles differ, first at {np.flatnonzero(diff)[:5]}"
        assert (got[12 * n:].view(np.uint32) == 0xFFFFFFFF).all() and (org[2 * n:] == -1).all(), "written beyond the range"
        if with_origins:
            assert (org[:2 * n].reshape(n, 2) == want_org).all()
        else:
            assert (org == -1).all()
        assert want_bad == S.NUM_BAD
        return want_bad

    bad = run(S.make_transforms(), meshes)
    assert ms.bad_indices() == bad == 10 and ms.bad_indices() == 0
    run(None, meshes)                                                  # the vertices as they are (-0.0 included)
    run(S.make_transforms(1), meshes, with_origins=False)
    assert ms.bad_indices() == 2 * bad                                 # two assemble calls since the last query
    # the scene holds addresses: rewrite the vertex tensors in place, assemble again
    meshes2 = S.make_meshes(variant=1)
    for (tv, _), (v2, _, _) in zip(tensors, meshes2):
        tv.copy_(torch.from_numpy(np.ascontiguousarray(v2, np.float32)))
    torch.cuda.synchronize()
    assert not same_tris(statement(meshes2, S.INSTANCE_MESH, None)[0], statement(meshes, S.INSTANCE_MESH, None)[0])
    run(S.make_transforms(2), meshes2)
    run(None, meshes2)
    assert ms.bad_indices() == 2 * bad
    ms.close()
    mem.free(d_tris); mem.free(d_org)


def test_stadium_mesh_assembled_on_the_device_builds_the_oracles_grid(mem):
    """one instance, no transform: the records of scene.tris_from_mesh; build_all on them gives the oracle's grid arrays, primary rays the oracle's hits"""
    import torch
    from hagrid_amd import api
    from oracle import oracle as O
    V, F = scene.make_stadium_mesh()
    tris = scene.tris_from_mesh(V, F)
    n = tris.shape[0]
    assert n > 900_000
    tV = torch.from_numpy(V).cuda(); tF = torch.from_numpy(F).cuda()
    torch.cuda.synchronize()
    ms = api.MeshScene(mem, [(tV.data_ptr(), V.shape[0], tF.data_ptr(), n)])
    d_tris = alloc_out(mem, 48 * n)
    ms.assemble(0, d_tris)
    assert ms.bad_indices() == 0
    assert fetch(mem, d_tris, np.float32, 12 * n).tobytes() == tris.tobytes()
    grid = api.build_all(mem, d_tris, n)
    G = O.Grid.full(tris)
    d = grid.download()
    assert grid.summary() == G.summary()
    assert (d["entries"] == G.entries).all() and (d["ref_ids"] == G.ref_ids).all() and d["cells"].tobytes() == G.cells.tobytes()
    rays = scene.make_rays_primary(grid.bbox_min, grid.bbox_max, 1024, 512)
    want, _ = G.traverse(tris, rays, nthreads=8)
    d_rays = mem.upload(rays); d_hits = alloc_out(mem, 16 * rays.shape[0])
    api.setup_traversal(grid)
    api.traverse_grid(grid, d_tris, d_rays, d_hits, rays.shape[0])
    hits = fetch(mem, d_hits, api.HIT_DTYPE, rays.shape[0])
    assert (hits["id"] == want["id"]).all() and (bits(hits["t"]) == bits(want["t"])).all()
    assert 0 < (want["id"] >= 0).sum()
    for p in (d_rays, d_hits, d_tris):
        mem.free(p)
    grid.free(); ms.close()


def test_frame_loop_on_one_stream_with_matrices_from_torch(mem):
    """four frames: torch computes the matrices on the device -> assemble -> build_all -> setup_traversal -> render_frame, all on torch's stream,
    no triangle or matrix crossing the bus in between; per frame the triangles are the statement's and the pixels the oracle's"""
    import torch
    from hagrid_amd import api
    from oracle import oracle as O
    V, F = scene.make_stadium_mesh(0.12)
    soup = scene.make_soup(5000)
    sv = np.ascontiguousarray(np.stack([soup[:, 0:3], soup[:, 0:3] - soup[:, 4:7], soup[:, 0:3] + soup[:, 8:11]], axis=1).reshape(-1, 3), np.float32)
    meshes = [(V, F, F.shape[0]), (sv, None, 5000)]
    instance_mesh = [0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    tensors, recs = to_device(meshes)
    w, h = 160, 120
    stream = torch.cuda.Stream()
    frames = []
    with torch.cuda.stream(stream):
        mem.use_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ms = api.MeshScene(mem, recs, instance_mesh)
            n = ms.num_tris
            assert n >= 100_000
            t_tris = torch.empty((n, 12), dtype=torch.float32, device="cuda")
            img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            ws = mem.alloc(api.frame_workspace_bytes(w, h, 0))
            k = torch.arange(len(instance_mesh), dtype=torch.float32, device="cuda")
            grid = None
            for frame in range(4):
                # the matrices of this frame, on the device: a turn about y that advances with the frame, an uneven scale, a place on a ring
                ang = 0.37 * k + 0.21 * frame
                c, s = torch.cos(ang), torch.sin(ang)
                sx, sy, sz = 0.8 + 0.05 * k, 1.1 - 0.03 * k, 0.9 + 0.01 * frame + 0.0 * k
                z0 = torch.zeros_like(k)
                M = torch.stack([c * sx, z0, s * sz, 2.5 * torch.cos(0.7 * k) + 0.1 * frame,
                                 z0, sy, z0, 0.3 * k,
                                 -s * sx, z0, c * sz, 2.5 * torch.sin(0.7 * k)], dim=1).contiguous()
                ms.assemble(M.data_ptr(), t_tris.data_ptr())
                if grid is not None:
                    grid.free()
                grid = api.build_all(mem, t_tris.data_ptr(), n)
                api.setup_traversal(grid)
                cam = scene.camera(grid.bbox_min, grid.bbox_max, ratio=w / float(h))
                api.render_frame(grid, t_tris.data_ptr(), cam, cam[4], w, h, ws, img.data_ptr(), mode=api.SHADE_DEPTH)
                # after the frame: what the oracle needs
                stream.synchronize()
                frames.append((M.cpu().numpy(), t_tris.cpu().numpy(), img.cpu().numpy().copy(), grid.bbox_min, grid.bbox_max))
            assert ms.bad_indices() == 0
            grid.free(); mem.free(ws); ms.close()
        finally:
            stream.synchronize()
            mem.use_stream(None)
    previous = None
    for frame, (M, got, px, lo, hi) in enumerate(frames):
        want, _, _ = statement(meshes, instance_mesh, M)
        assert same_tris(got, want), frame
        assert previous is None or not same_tris(previous, want), "the scene did not move"
        previous = want
        G = O.Grid.full(want)
        assert (bits(G.bbox_min) == bits(lo)).all() and (bits(G.bbox_max) == bits(hi)).all()
        rays = scene.make_rays_primary(lo, hi, w, h)
        oh, _ = G.traverse(want, rays, nthreads=8)
        assert (px.reshape(-1, 4) == scene.shade_hits(oh, scene.SHADE_DEPTH, float(rays[0, 7]))).all(), frame
        assert 0 < (oh["id"] >= 0).sum() < w * h


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_cpp_api import _build_cli
    d = tmp_path_factory.mktemp("assemble_cli")
    return _build_cli(str(d)), d


def _grid_file_tris(path):
    from hagrid_amd import lib
    data = open(path, "rb").read()
    hd = lib.BlobHeader.from_buffer_copy(data[:C.sizeof(lib.BlobHeader)])
    return np.frombuffer(data, np.float32, 12 * hd.num_tris, hd.off_tris).reshape(hd.num_tris, 12)


def test_cli_device_tris_writes_the_same_grid_file(cli):
    exe, d = cli
    V, F = scene.make_stadium_mesh()
    obj = str(d / "stadium.obj")
    scene.write_obj(obj, V, F)
    for name, model in (("stadium", obj), ("soup", "soup:20000")):
        host_file, dev_file = str(d / (name + "_host.grid")), str(d / (name + "_dev.grid"))
        r0 = _subproc.check([exe, model, "-sx", "64", "-sy", "64", "--save-grid", host_file], timeout=300)
        r1 = _subproc.check([exe, model, "-sx", "64", "-sy", "64", "--device-tris", "--save-grid", dev_file], timeout=300)
        a, b = open(host_file, "rb").read(), open(dev_file, "rb").read()
        assert len(a) > 256 and a == b, name
        line = lambda r, key: [l for l in r.stdout.splitlines() if key in l]
        assert line(r0, "triangle(s)") == line(r1, "triangle(s)") and line(r0, "intersection(s)") == line(r1, "intersection(s)")
    assert same_tris(_grid_file_tris(str(d / "stadium_dev.grid")), scene.tris_from_mesh(V, F))
    assert same_tris(_grid_file_tris(str(d / "soup_dev.grid")), scene.make_soup(20000))
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--device-tris" in r.stdout and r.stdout.index("--device-tris") > r.stdout.index("--bench-warmup")
    assert r.stdout.index("--device-tris") > r.stdout.index("Extensions of this front-end")


def test_argument_errors_zero_triangles_and_memory(mem):
    from hagrid_amd import api, lib
    L, ctx = mem._L, mem._ctx
    EINVAL, ERANGE = -1, -4
    buf = mem.alloc(4096)
    vp = C.c_void_p

    def mesh(vertices=buf, indices=buf + 1024, nv=16, nt=8, stride=12, reserved=0):
        m = lib.Mesh()
        m.vertices, m.indices, m.num_vertices, m.num_tris, m.vertex_stride, m.reserved = vertices or None, indices or None, nv, nt, stride, reserved
        return m

    def create(meshes, inst, n_inst=None, num_meshes=None, null_out=False):
        arr = (lib.Mesh * max(len(meshes), 1))(*meshes)
        ia = (C.c_int32 * max(len(inst), 1))(*inst) if inst is not None else None
        out = vp(0xDEAD)
        rc = L.hagrid_scene_create(ctx, arr if meshes else None, len(meshes) if num_meshes is None else num_meshes, ia,
                                   (len(inst) if inst is not None else len(meshes)) if n_inst is None else n_inst, None if null_out else C.byref(out))
        return rc, out

    def refused(code, text, *a, **kw):
        rc, out = create(*a, **kw)
        assert rc == code, (rc, text)
        assert not out.value, "*out must be NULL after an error"
        msg = L.hagrid_last_error(ctx)
        assert msg and text.encode() in msg, (text, msg)

    usage0 = mem.usage()
    refused(EINVAL, "stride", [mesh(stride=8)], None)
    refused(EINVAL, "stride", [mesh(stride=14)], None)
    refused(EINVAL, "negative", [mesh(nv=-1)], None)
    refused(EINVAL, "negative", [mesh(nt=-1)], None)
    refused(EINVAL, "negative", [mesh()], [0], n_inst=-1)
    refused(EINVAL, "negative", [mesh()], None, num_meshes=-1, n_inst=-1)
    refused(EINVAL, "reserved", [mesh(reserved=1)], None)
    refused(EINVAL, "without vertices", [mesh(nv=0, nt=1)], None)
    refused(EINVAL, "null vertex buffer", [mesh(vertices=0)], None)
    refused(EINVAL, "4-byte aligned", [mesh(vertices=buf + 2)], None)
    refused(EINVAL, "4-byte aligned", [mesh(indices=buf + 1025)], None)
    refused(EINVAL, "outside the mesh array", [mesh()], [0, 1])
    refused(EINVAL, "outside the mesh array", [mesh()], [-1])
    refused(EINVAL, "one instance per mesh", [mesh(), mesh()], None, n_inst=1)
    refused(EINVAL, "without indices", [mesh(indices=0, nv=2 ** 31 - 1, nt=2 ** 30)], None)
    rc, _ = create([], None, num_meshes=2)                       # null mesh array
    assert rc == EINVAL and b"null mesh array" in L.hagrid_last_error(ctx)
    rc, _ = create([mesh()], None, null_out=True)
    assert rc == EINVAL and b"null output" in L.hagrid_last_error(ctx)
    refused(ERANGE, "2^31 - 1", [mesh(nv=2 ** 31 - 1, nt=2 ** 30)], [0, 0])     # 2^31 output triangles (nothing is launched, nothing is read)
    assert mem.usage() == usage0
    assert L.hagrid_scene_first_tri(None, 0) == EINVAL

    # a real scene for the assemble-time errors
    rc, sc = create([mesh()], [0, 0])
    assert rc == 0 and sc.value
    assert L.hagrid_scene_first_tri(sc, 2) == 16 and L.hagrid_scene_first_tri(sc, 3) == EINVAL and L.hagrid_scene_first_tri(sc, -1) == EINVAL
    out = mem.alloc(48 * 16 + 64)
    assert L.hagrid_scene_assemble(ctx, None, None, vp(out), None) == EINVAL
    assert L.hagrid_scene_assemble(ctx, sc, None, None, None) == EINVAL and b"null triangle buffer" in L.hagrid_last_error(ctx)
    assert L.hagrid_scene_assemble(ctx, sc, None, vp(out + 4), None) == EINVAL and b"16-byte aligned" in L.hagrid_last_error(ctx)
    assert L.hagrid_scene_assemble(ctx, sc, vp(buf + 2), vp(out), None) == EINVAL and b"4-byte aligned" in L.hagrid_last_error(ctx)
    assert L.hagrid_scene_assemble(ctx, sc, None, vp(out), vp(buf + 2050)) == EINVAL and b"origins must be 4-byte aligned" in L.hagrid_last_error(ctx)
    assert L.hagrid_scene_bad_indices(ctx, sc, None) == EINVAL
    n = C.c_int64(-1)
    assert L.hagrid_scene_bad_indices(ctx, None, C.byref(n)) == EINVAL and b"null scene" in L.hagrid_last_error(ctx)
    other = api.MemManager(keep=False)                           # a scene is used with the context it was created in
    try:
        assert L.hagrid_scene_assemble(other._ctx, sc, None, vp(out), None) == EINVAL and b"another context" in L.hagrid_last_error(other._ctx)
        assert L.hagrid_scene_bad_indices(other._ctx, sc, C.byref(n)) == EINVAL and b"another context" in L.hagrid_last_error(other._ctx)
    finally:
        other.close()
    L.hagrid_scene_destroy(ctx, sc)
    L.hagrid_scene_destroy(ctx, None)                             # a no-op
    mem.free(out)
    with pytest.raises(api.HagridError):
        api.MeshScene(mem, [(buf, 16, 0, 8, 10)])

    # zero triangles: fine, and nothing is launched or written (a null triangle buffer is accepted)
    for meshes, inst in (([], []), ([mesh(nt=0)], [0, 0, 0]), ([mesh()], [])):
        rc, sc = create(meshes, inst)
        assert rc == 0 and sc.value
        assert L.hagrid_scene_first_tri(sc, len(inst)) == 0
        assert L.hagrid_scene_assemble(ctx, sc, None, None, None) == 0
        assert L.hagrid_scene_bad_indices(ctx, sc, C.byref(n)) == 0 and n.value == 0
        L.hagrid_scene_destroy(ctx, sc)
    mem.free(buf)

    # the scene's tables are pool memory: usage returns to its former value after destroy (keep = false)
    m2 = api.MemManager(keep=False)
    try:
        b2 = m2.alloc(4096)
        before = m2.usage()
        ms = api.MeshScene(m2, [(b2, 16, 0, 5)], [0] * 1000)
        assert ms.num_tris == 5000 and m2.usage() > before
        ms.close()
        assert m2.usage() == before
        m2.free(b2)
    finally:
        m2.close()

    # the context still assembles
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    d_v = mem.upload(v); d_t = alloc_out(mem, 48)
    ms = api.MeshScene(mem, [(d_v, 3, 0, 1)])
    ms.assemble(0, d_t)
    assert same_tris(fetch(mem, d_t, np.float32, 12).reshape(1, 12), scene.tris_from_vertices(v[0:1], v[1:2], v[2:3]))
    ms.close(); mem.free(d_v); mem.free(d_t)
