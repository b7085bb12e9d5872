"""The scene the assemble tests share (tests/test_assemble_cpu.py, tests/test_assemble_gpu.py): five meshes, thirteen instances.

  mesh 0  indexed, stride 12, 130 triangles (not a multiple of 64); three of its triangles name a vertex out of range (-1, V, 2^31 - 1)
  mesh 1  no indices (triangle p = vertices 3p, 3p+1, 3p+2), 7 triangles; one coordinate is -0.0
  mesh 2  indexed, stride 16 (a (V, 4) array whose fourth column is garbage), 200 triangles
  mesh 3  vertices but no triangles
  mesh 4  indexed, 3 triangles; one names vertex V (out of range)
Instances: 0 1 1 4 1 3 4 2 0 1 4 4 2 -- mesh 1 and mesh 4 placed several times, six instances of 7, 7, 3, 7, 0, 3 triangles in a row (one
wavefront covers five instance boundaries), the empty one among them.  Matrices: rotations about three axes, uneven scales, a mirror and
translations multiplied together in float64 and rounded to float32 -- their entries and the vertex coordinates are 24-bit values whose
products are not representable, so a fused multiply-add gives other bits (fma_would_differ() shows that it does)."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hagrid_amd import scene  # noqa: E402

INSTANCE_MESH = [0, 1, 1, 4, 1, 3, 4, 2, 0, 1, 4, 4, 2]


def _verts(seed, n, cols=3):
    u = scene.uniform01(seed, np.arange(n * cols, dtype=np.uint64)).reshape(n, cols)
    return (np.float32(2.0) * u - np.float32(1.0)).astype(np.float32)


def _faces(seed, nf, nv):
    u = scene.uniform01(seed, np.arange(nf * 3, dtype=np.uint64)).reshape(nf, 3)
    return np.minimum((u * np.float32(nv)).astype(np.int32), nv - 1).astype(np.int32)


def make_meshes(variant=0):
    """[(vertices (V, 3 | 4) float32, faces (F, 3) int32 | None, F)]; `variant` draws other vertices (the same faces): a second frame."""
    s = 1000 * variant
    f0 = _faces(11, 130, 40); f0[5, 1] = -1; f0[77, 0] = 40; f0[129, 2] = 2 ** 31 - 1
    v1 = _verts(s + 2, 21); v1[4, 1] = np.float32(-0.0); v1[9, 0] = np.float32(-0.0)
    v2 = _verts(s + 3, 57, cols=4); v2[:, 3] = np.float32(1e30)
    f4 = _faces(14, 3, 6); f4[1, 2] = 6
    return [(_verts(s + 1, 40), f0, 130), (v1, None, 7), (v2, _faces(13, 200, 57), 200), (_verts(s + 5, 4), np.zeros((0, 3), np.int32), 0), (_verts(s + 6, 6), f4, 3)]


BAD_PER_MESH = [3, 0, 0, 0, 1]
NUM_BAD = sum(BAD_PER_MESH[k] for k in INSTANCE_MESH)


def make_transforms(frame=0):
    """(13, 12) float32: per instance rotate * scale * mirror, then translate; `frame` turns everything a little further"""
    out = np.empty((len(INSTANCE_MESH), 12), np.float32)
    for i in range(len(INSTANCE_MESH)):
        a, b, c = 0.37 + 0.61 * i + 0.05 * frame, 1.13 - 0.29 * i, 0.71 * i + 0.11 * frame
        rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        sc = np.diag([0.3 + 0.17 * i, 1.9 - 0.11 * i, 0.77])
        mirror = np.diag([-1.0 if i % 3 == 1 else 1.0, 1.0, 1.0])
        m = rx @ ry @ rz @ sc @ mirror
        t = np.array([0.9 * i - 3.1, 0.123 * i * i, -0.456 * i + 0.01 * frame])
        out[i] = np.concatenate([m, t[:, None]], axis=1).astype(np.float32).reshape(12)
    return out


def fma_would_differ(meshes, transforms):
    """True when contracting the first product-sum of the transform (M[0]*x + M[1]*y -> fma(M[1], y, M[0]*x)) changes a bit somewhere"""
    for i, k in enumerate(INSTANCE_MESH):
        v = meshes[k][0]; m = transforms[i]
        plain = (m[0] * v[:, 0] + m[1] * v[:, 1]).astype(np.float32)
        fused = (np.float64(m[1]) * v[:, 1].astype(np.float64) + (m[0] * v[:, 0]).astype(np.float64)).astype(np.float32)      # exact product, one rounding
        if (plain.view(np.uint32) != fused.view(np.uint32)).any():
            return True
    return False


def write_scene_file(path, meshes, instance_mesh, transforms):
    """the input format of tests/cpp/assemble_host.cpp"""
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", len(meshes), len(instance_mesh), 0 if transforms is None else 1))
        for v, faces, nf in meshes:
            f.write(struct.pack("<4i", v.shape[0], nf, 4 * v.shape[1], 0 if faces is None else 1))
        for v, faces, nf in meshes:
            f.write(np.ascontiguousarray(v, np.float32).tobytes())
            if faces is not None:
                f.write(np.ascontiguousarray(faces, np.int32).tobytes())
        f.write(np.asarray(instance_mesh, np.int32).tobytes())
        if transforms is not None:
            f.write(np.ascontiguousarray(transforms, np.float32).tobytes())


def read_host_output(path):
    data = open(path, "rb").read()
    bad = struct.unpack("<q", data[:8])[0]
    n = (len(data) - 8) // 56
    tris = np.frombuffer(data, np.float32, 12 * n, 8).reshape(n, 12)
    origins = np.frombuffer(data, np.int32, 2 * n, 8 + 48 * n).reshape(n, 2)
    return tris, origins, bad
