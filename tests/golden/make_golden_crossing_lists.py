"""Writes tests/golden/crossing_lists.npz: the complete sorted crossing lists of exactly the rays stored in tests/golden/crossings.npz (three scenes), for
tests/test_crossing_lists_cpu.py and tests/test_crossing_lists_gpu.py.

Needs oracle/_ref/libhagrid_ref.so, which oracle/Makefile compiles where a checkout of the reference project is at hand:

    make -C oracle && python tests/golden/make_golden_crossing_lists.py

ACCEPT and t of every (ray, triangle) pair come from the REFERENCE's arithmetic, one triangle at a time (make_golden_crossings.py: reference_pairs); the
FACING comes from scene.ray_tri_pairs, whose accept and t are asserted equal to the reference's on every pair, bit for bit.  The pairs of a ray sorted by
(t, id) are its list.  Asserted before anything is written:
  * the records made from the lists by tests/_crossings.py: records_from_pairs equal the records of crossings.npz, bit for bit;
  * for soup and mesh, the first min(m, 8) entries of every ray equal multi_hit.npz in id and t;
  * scene.ray_crossing_lists gives the same lists.

Output keys, per scene s in soup, mesh, solids (the rays are those of crossings.npz and are not stored again):
  <s>_offsets   int64  [n + 1]     ray i owns the entries offsets[i] .. offsets[i+1]
  <s>_t         uint32 [total]     the bits of t
  <s>_key       int32  [total]     id * 2 + entering
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _crossings as X  # noqa: E402
import _crossing_lists as CL  # noqa: E402
import _multi_hit as M  # noqa: E402
from hagrid_amd import scene  # noqa: E402
from make_golden_crossings import reference_pairs  # noqa: E402


def lists_by_reference(tris, rays):
    r, j, t = reference_pairs(tris, rays)
    pairs = scene.ray_tri_pairs(tris[j], rays[r])
    assert pairs["accept"].all(), "numpy refuses a pair the reference accepts"
    assert (pairs["t"].view(np.uint32) == t.view(np.uint32)).all(), "numpy's t differs from the reference's"
    entering = pairs["entering"]
    order = np.lexsort((j, t, r))
    offsets = np.zeros(rays.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=rays.shape[0]), out=offsets[1:])
    return (r, j, t, entering), (offsets, t[order].astype(np.float32), (j[order] * 2 + entering[order]).astype(np.int32))


def main():
    from oracle import oracle as O
    if O.ref_lib() is None:
        raise SystemExit("oracle/_ref/libhagrid_ref.so is missing: this fixture is made from the reference's headers")
    have = np.load(X.FIXTURE)
    mh = np.load(M.FIXTURE)
    out = {}
    for name in X.SCENES:
        tris = X.make_tris(name)
        rays = have[name + "_rays"]
        (r, j, t, entering), (offsets, lt, key) = lists_by_reference(tris, rays)
        rec = X.records_from_pairs(rays, r, j, t, entering)
        assert (X.rec_bits(rec) == have[name + "_records"]).all(), f"{name}: the records made from the lists differ from crossings.npz"
        assert ((offsets[1:] - offsets[:-1]) == have[name + "_records"][:, 0].view(np.int32)).all()
        if name in M.SCENES:
            ids, ts = mh[name + "_ids"], mh[name + "_t"]
            for i in range(ids.shape[0]):
                k = min(int(offsets[i + 1] - offsets[i]), 8)
                a = int(offsets[i])
                assert (key[a:a + k] >> 1 == ids[i, :k]).all() and (ids[i, k:] < 0).all(), f"{name}: ray {i}: the first {k} ids differ from multi_hit.npz"
                assert (lt[a:a + k].view(np.uint32) == M.bits(ts[i, :k])).all(), f"{name}: ray {i}: the first {k} t differ from multi_hit.npz"
        mo, mt, mk = scene.ray_crossing_lists(tris, rays)
        assert (mo == offsets).all() and (mt.view(np.uint32) == lt.view(np.uint32)).all() and (mk == key).all(), f"{name}: scene.ray_crossing_lists differs"
        print(name, tris.shape[0], "triangles,", rays.shape[0], "rays,", int(offsets[-1]), "crossings, the longest list", int((offsets[1:] - offsets[:-1]).max()))
        out[name + "_offsets"] = offsets; out[name + "_t"] = lt.view(np.uint32); out[name + "_key"] = key
    np.savez_compressed(CL.FIXTURE, **out)
    print(CL.FIXTURE, os.path.getsize(CL.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
