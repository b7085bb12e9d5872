"""The scenes and traversal-image formats that tests/test_traverse_gpu.py and tests/test_hostile_rays_gpu.py run the image kernels on."""
import numpy as np

from hagrid_amd import scene


def image_scenes():
    sparse = scene.make_soup(3000, seed=5).copy()                      # two clusters far apart: top-level cells without subdivision
    sparse[:1500, 0:3] *= np.float32(0.2); sparse[1500:, 0:3] = sparse[1500:, 0:3] * np.float32(0.2) + np.float32(3.0)
    coincident = np.repeat(scene.make_soup(40, seed=6), 30, axis=0)    # lists far longer than four references
    return {"soup20k": (scene.make_soup(20000), {}), "soup30k_shift3": (scene.make_soup(30000, seed=11), dict(top_density=0.15, snd_density=3.0)),
            "dense_wide": (scene.make_soup(8000, seed=12), dict(top_density=0.08, snd_density=10.0)),     # a top-level cell with > 255 cells
            "deep": (scene.make_soup(6000, seed=12), dict(top_density=0.01, snd_density=40.0)),   # shift 5: blocks stop at depth 3, deep links below
            "sparse": (sparse, {}), "coincident": (np.concatenate([coincident, scene.make_soup(2000, seed=7)]), {}),
            "tiny": (scene.make_soup(3, seed=8), {}),
            "compressed": (scene.make_soup(20000, seed=14), dict(compress=True)),
            "compressed_deep": (scene.make_clustered(3000, 3, 4000), dict(compress=True)),          # shift 5, SmallCells: blocks + nested blocks, no deep links
            "compressed_long_lists": (np.concatenate([np.repeat(scene.make_soup(30, seed=15), 12, axis=0), scene.make_soup(6000, seed=16)]), dict(compress=True, top_density=0.3, snd_density=1.0))}


# (traverse.image, traverse.image_slim, traverse.image_general): the traversal image holds 16-byte slim records in one of three layouts -- grids of at most three
# levels: a block of records per top-level cell, table-free where (nearly) every top-level cell has the full depth (uniform layout), through the table otherwise
# (table layout; wide records for cells whose bounds do not fit a byte); every other grid a record per voxel-map entry (general layout: any depth, links to child
# blocks, wide records).  "image1": the value 1 of the option (round 1-4's compact form) builds the same image as 2; the 26-bit form of the record; the general
# layout forced on grids the block layouts would serve
IMAGE_FORMATS = {"flat": (2, 1, 1), "image1": (1, 1, 1), "flat_slim26": (2, 2, 1), "flat_general": (2, 1, 2)}
