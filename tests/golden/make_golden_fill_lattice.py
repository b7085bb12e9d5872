"""Writes tests/golden/fill_lattice.npz: hagrid_fill_lattice by its numpy definition (scene.fill_lattice) on the lattices of tests/_fill_lattice.py, for
tests/test_fill_lattice_cpu.py and tests/test_fill_lattice_gpu.py.

    python tests/golden/make_golden_fill_lattice.py

Needs nothing but numpy: scene.fill_lattice stands on scene.ray_crossing_lists and scene.ray_crossings, which tests/golden/crossing_lists.npz and crossings.npz
pin against the reference's arithmetic.  Asserted before anything is written: the records of an axis do not depend on the mask or the vote rule, and the rows
of a mask are the rows of its axes.

Output keys, per lattice k (tests/_fill_lattice.py: all_cases):
  <k>_origin, <k>_size   float32 [3]
  <k>_n                  int32   [3]
  <k>_inside             int8    [2, 7, voxels]     vote rule (0 parity, 1 winding) x axis mask 1 .. 7; x fastest
  <k>_records            uint32  [rows, 4]          the records of the row rays of ALL three axes, axis after axis, the lower remaining axis fastest
  <k>_abstained          uint8   [2, rows]          vote rule x row: 1 when the row ends inside
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import _crossings as X  # noqa: E402
import _fill_lattice as FL  # noqa: E402
from hagrid_amd import scene  # noqa: E402


def main():
    out = {}
    tris_of = {}
    for name, key, origin, size, n in FL.all_cases():
        tris = tris_of.setdefault(name, FL.make_tris(name))
        voxels = int(np.prod(n))
        inside = np.zeros((2, 7, voxels), np.int8)
        rows = sum(FL.row_counts(n))
        records = np.zeros((rows, 4), np.uint32)
        abstained = np.zeros((2, rows), np.uint8)
        seen = np.zeros(rows, bool)
        for w in (0, 1):
            for mask in FL.MASKS:
                r = scene.fill_lattice(tris, origin, size, n, axes=mask, winding=bool(w))
                assert r["inside"].min() >= -1 and r["inside"].max() <= 1
                inside[w, mask - 1] = r["inside"]
                idx = FL.rows_of_mask(n, mask)
                bits = X.rec_bits(r["records"])
                assert idx.size == bits.shape[0] == r["abstained"].size
                assert (records[idx][seen[idx]] == bits[seen[idx]]).all(), "the records of a row depend on the mask or the rule"
                records[idx] = bits
                if mask in (1, 2, 4):
                    abstained[w, idx] = r["abstained"]
                assert (abstained[w, idx] == r["abstained"]).all() or mask in (1, 2, 4), "the abstaining rows depend on the mask"
                seen[idx] = True
        print(key, tris.shape[0], "triangles,", tuple(int(v) for v in n), "voxels", voxels, "rows", rows, "most crossings", int(records[:, 0].max()),
              "abstaining rows (parity, winding)", abstained.sum(axis=1).tolist(), "voxels at -1 with all axes", [(inside[w, 6] < 0).sum() for w in (0, 1)])
        out[key + "_origin"] = np.asarray(origin, np.float32); out[key + "_size"] = np.asarray(size, np.float32); out[key + "_n"] = np.asarray(n, np.int32)
        out[key + "_inside"] = inside; out[key + "_records"] = records; out[key + "_abstained"] = abstained
    np.savez_compressed(FL.FIXTURE, **out)
    print(FL.FIXTURE, os.path.getsize(FL.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
