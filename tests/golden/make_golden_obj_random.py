"""Writes tests/golden/obj_random_golden.npz: random OBJ face soups and MTL command soups, and what the REFERENCE's own
readers make of them, for tests/test_obj_loader.py.

Needs oracle/_ref/libhagrid_ref_obj.so, which oracle/Makefile compiles where a checkout of the reference project is at hand
(see make_golden_obj.py):

    make -C oracle && python tests/golden/make_golden_obj_random.py

Output keys, per case i:
  obj_text_<i>  the OBJ file (random face soup: polygons of 3..12 corners, mixed index forms, negative indices), 20 cases
  obj_n_<i>     what ref_load_model returned (triangle count, -1 = refused)
  obj_tris_<i>  float32 [n, 12]: the Tri records it produced
  mtl_text_<i>  the MTL file (random commands: valid, malformed, unknown; CRLF on every third), 30 cases
  mtl_out_<i>   the material library the reference's load_mtl read, as the text ref_load_mtl prints (bytes)
"""
import ctypes as C
import os
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def obj_cases():
    rng = np.random.default_rng(5)
    texts = []
    for case in range(20):
        nv = int(rng.integers(3, 60))
        lines = []
        have = 0
        for _ in range(int(rng.integers(1, 40))):
            add = int(rng.integers(0, 4))
            for _ in range(add):
                if have < nv:
                    lines.append("v %r %r %r" % tuple(float(x) for x in rng.normal(size=3).astype(np.float32))); have += 1
            if have < 3:
                continue
            k = int(rng.integers(3, 13))
            corners = []
            for _ in range(k):
                i = int(rng.integers(1, have + 1))
                if rng.random() < 0.3: i = i - have - 1
                form = rng.integers(0, 4)
                corners.append([f"{i}", f"{i}/1", f"{i}//1", f"{i}/1/1"][form])
            lines.append(("f " if rng.random() < 0.8 else "f\t") + " ".join(corners))
            if rng.random() < 0.1: lines.append("g part%d" % case)
            if rng.random() < 0.05: lines.append("o obj%d" % case)
        texts.append("vn 0 0 1\nvt 0 0\n" + "\n".join(lines) + "\n")
    return texts


def mtl_cases():
    rng = np.random.default_rng(11)
    cmds = ["newmtl", "Ka", "Kd", "Ks", "Ke", "Ns", "Ni", "Tf", "Tr", "d", "illum", "map_Ka", "map_Kd", "map_Ks", "map_Ke", "map_bump", "bump", "map_d",
            "Kq", "N", "Tz", "dd", "illu", "map_K", "#", "usemtl", ""]
    texts = []
    for case in range(30):
        lines = []
        for _ in range(int(rng.integers(1, 40))):
            c = cmds[int(rng.integers(0, len(cmds)))]
            sep = [" ", "\t", "  ", ""][int(rng.integers(0, 4))]
            kind = rng.integers(0, 4)
            if kind == 0: arg = " ".join("%r" % float(x) for x in rng.normal(size=int(rng.integers(0, 5))).astype(np.float32))
            elif kind == 1: arg = "m%d" % int(rng.integers(0, 4))
            elif kind == 2: arg = "some file %d.png  " % int(rng.integers(0, 9))
            else: arg = ""
            lines.append(["", " ", "\t "][int(rng.integers(0, 3))] + c + sep + arg)
        texts.append(("\r\n" if case % 3 == 0 else "\n").join(lines) + ("\n" if case % 2 else ""))
    return texts


def main():
    R = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libhagrid_ref_obj.so"))
    R.ref_load_model.restype = C.c_int; R.ref_load_model.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
    R.ref_load_mtl.restype = C.c_int; R.ref_load_mtl.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for i, text in enumerate(obj_cases()):
            p = os.path.join(d, f"r{i}.obj")
            with open(p, "w", newline="") as f:
                f.write(text)
            buf = np.zeros((8192, 12), np.float32)
            n = R.ref_load_model(p.encode(), buf.ctypes.data, buf.shape[0])
            out[f"obj_text_{i}"] = np.frombuffer(text.encode(), np.uint8)
            out[f"obj_n_{i}"] = np.int32(n)
            out[f"obj_tris_{i}"] = buf[:max(n, 0)].copy()
        for i, text in enumerate(mtl_cases()):
            p = os.path.join(d, f"r{i}.mtl")
            with open(p, "w", newline="") as f:
                f.write(text)
            buf = C.create_string_buffer(1 << 16)
            n = R.ref_load_mtl(p.encode(), buf, len(buf))
            assert n >= 0, i
            out[f"mtl_text_{i}"] = np.frombuffer(text.encode(), np.uint8)
            out[f"mtl_out_{i}"] = np.frombuffer(buf.raw[:n], np.uint8)
    np.savez_compressed(os.path.join(HERE, "obj_random_golden.npz"), **out)
    print(f"wrote obj_random_golden.npz: {len(obj_cases())} OBJ and {len(mtl_cases())} MTL cases")


if __name__ == "__main__":
    main()
