"""What the helper modules of the queries over the construction format (_closest, _overlap, _crossings, _multi_hit) share: how a host program of tests/cpp
is built, how arrays and the grid reach it as files (tests/cpp/host_support.h reads them), and the grids of the CPU oracle they walk.  What the GPU test files of the same queries share
(the case on the device, the checks around a query's launches, the shim build, the kernel budget) is tests/_gpu_case.py."""
import os
import re
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def build_host(name: str, directory, sanitize: bool = False) -> str:
    """tests/cpp/<name>.cpp as a program in `directory`; sanitize: a stand-alone binary <name>_san with the sanitizers of SANITIZE"""
    exe = os.path.join(str(directory), name + ("_san" if sanitize else ""))
    subprocess.run(["g++", "-std=c++11", *(SANITIZE if sanitize else ["-O2"]), "-Wall", "-ffp-contract=off", "-DHOST=", "-DDEVICE=", "-I", INC,
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe], check=True)
    return exe


def put(directory, name, arr) -> str:
    path = os.path.join(str(directory), name + ".bin")
    np.ascontiguousarray(arr).tofile(path)
    return path


def is_small(grid: dict) -> bool:
    return grid.get("small_cells") is not None


def grid_header(grid: dict) -> bytes:
    """what a walk's parameter file says of the grid (keys bbox_min, bbox_max, dims, shift, cells | small_cells: what api.Grid.download returns):
    i32 small, 3 i32 top-level dims, i32 shift, 3 f32 bbox min, 3 f32 bbox max"""
    return struct.pack("<i3ii3f3f", 1 if is_small(grid) else 0, *[int(v) for v in grid["dims"]], int(grid["shift"]),
                       *[float(v) for v in grid["bbox_min"]], *[float(v) for v in grid["bbox_max"]])


def grid_files(directory, grid: dict, prefix: str = "") -> list:
    """the files ENTRIES CELLS REFS of a walk (keys entries, ref_ids, cells | small_cells)"""
    return [put(directory, prefix + "entries", grid["entries"]), put(directory, prefix + "cells", grid["small_cells"] if is_small(grid) else grid["cells"]),
            put(directory, prefix + "refs", grid["ref_ids"])]


def oracle_grid_arrays(G) -> dict:
    """the arrays of an oracle.Grid in the shape the host walks take"""
    return {"entries": np.array(G.entries), "ref_ids": np.array(G.ref_ids), "cells": None if G.cells is None else np.array(G.cells),
            "small_cells": None if G.small_cells is None else np.array(G.small_cells),
            "bbox_min": G.bbox_min, "bbox_max": G.bbox_max, "dims": G.dims, "shift": G.shift}


def oracle_grid(tris: np.ndarray, compress: bool, subset_only: bool):
    """the construction sequence of the CPU oracle with either expansion mode"""
    from oracle import oracle as O
    G = O.Grid.build(tris).merge().flatten().expand(tris, 3, subset_only=subset_only)
    if compress:
        G.compress()
    return G


def kernel_rows(unit: str) -> dict:
    """tools/kernel_resources.py for one translation unit: kernel name -> (VGPRs, spilled VGPRs, scratch bytes, wavefronts per SIMD)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), unit], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"vgpr\s+(\d+) spill\s+(\d+) scratch\s+(\d+) .* occ (\d+)\s+.*::(\w+_kernel)\(", line)
        if m:
            rows[m.group(5)] = tuple(int(m.group(i)) for i in (1, 2, 3, 4))
    print(r.stdout)
    return rows


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
