"""Writes tests/golden/distance_lattice.npz from scene.distance_lattice (the numpy statement: closest_points over lattice_centres with r = band) only.
Per lattice `key` of tests/_distance.py and per band (1.5 and 3 largest voxel edges): key_id int32, key_d2 float32, key_q float32 x 3, key_feature int8,
key_side int8 -- arrays with the band as their first axis --, key_band float32[2], key_pairs int64[2] (pairs within the band) and key_n int32[3].
usage: python tests/golden/make_golden_distance_lattice.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from hagrid_amd import scene  # noqa: E402
import _distance as D  # noqa: E402


def main():
    out = {}
    for name, key, origin, size, n in D.all_cases():
        tris = D.tris_of(name)
        recs, bands, pairs = [], [], []
        for f in D.BAND_FACTORS:
            band = D.band_of(size, f)
            recs.append(scene.distance_lattice(tris, origin, size, n, band))
            bands.append(band); pairs.append(D.pairs_within(tris, origin, size, n, band))
            found = (recs[-1]["id"] >= 0).mean()
            print(f"{key}: {tris.shape[0]} triangles, {recs[-1].size} voxels, band {float(band):.6g}: share found {found:.3f}, {pairs[-1] / recs[-1].size:.1f} pairs within the band per voxel")
        out[key + "_id"] = np.stack([r["id"] for r in recs]).astype(np.int32)
        out[key + "_d2"] = np.stack([r["d2"] for r in recs]).astype(np.float32)
        out[key + "_q"] = np.stack([r["q"] for r in recs]).astype(np.float32)
        out[key + "_feature"] = np.stack([r["feature"] for r in recs]).astype(np.int8)
        out[key + "_side"] = np.stack([r["side"] for r in recs]).astype(np.int8)
        out[key + "_band"] = np.asarray(bands, np.float32)
        out[key + "_pairs"] = np.asarray(pairs, np.int64)
        out[key + "_n"] = np.asarray(n, np.int32)
    np.savez_compressed(D.FIXTURE, **out)
    print(D.FIXTURE, os.path.getsize(D.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
