"""RayZen's own BVH.cpp and Mesh.cpp, compiled as they stand and driven from Python -- the reference itself, run here.

TEST INFRASTRUCTURE ONLY, and only usable where the reference checkout is (the build container): the two sources and their
headers are read from /root/reference at BUILD time, never copied; the shared library lands in oracle/_ref/cppref/ (git-ignored).
The GPU box has neither; tests there use the fixtures this module generated (tests/golden/cppref_*.npz, made by
tests/golden/make_cppref.py).  What is and is not pinned by this: oracle/cppref/README.md.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
REF_DIR = os.path.join(os.path.dirname(_HERE), "_ref", "cppref")            # oracle/_ref/: git-ignored build outputs
LIBRARY = os.path.join(REF_DIR, "libcppref.so")
RAYZEN = "/root/reference/RayZen"
SOURCES = ("src/BVH.cpp", "src/Mesh.cpp")
HEADERS = ("include/BVH.h", "include/Mesh.h", "include/Logger.h")

TRIANGLE = np.dtype([("v0", "<f4", 3), ("pad0", "<f4"), ("v1", "<f4", 3), ("pad1", "<f4"),
                     ("v2", "<f4", 3), ("pad2", "<f4"), ("materialIndex", "<i4"), ("tail", "<i4", 3)])
NODE = np.dtype([("bmin", "<f4", 3), ("leftFirst", "<i4"), ("bmax", "<f4", 3), ("count", "<i4")])
MIDPOINT, SAH = 0, 1                                                          # BVHSplitMethod


def available():
    """The reference's C++ sources and headers are here (true in the build container only)."""
    return all(os.path.exists(os.path.join(RAYZEN, f)) for f in SOURCES + HEADERS)


def built():
    return os.path.exists(LIBRARY)


def _cxx_flags():
    from rayzen_amd import build as b          # the host library's flags: what the product's builder is compiled with
    return [f for f in b.CXX_FLAGS if f not in ("-Wall", "-Wextra")]          # (the reference's warnings are not ours to read)


def build(force=False, glm_dir=None, out=None):
    """g++ <the host library's CXX_FLAGS> BVH.cpp Mesh.cpp cppref_driver.cpp -> oracle/_ref/cppref/libcppref.so.
    glm_dir / out: compile against another stand-in into another file (how the README's two mutation experiments were run)."""
    out = out or LIBRARY
    glm_dir = glm_dir or _HERE
    mine = [os.path.join(_HERE, "cppref_driver.cpp"), os.path.join(glm_dir, "glm", "glm.hpp"), os.path.abspath(__file__)]
    theirs = [os.path.join(RAYZEN, f) for f in SOURCES + HEADERS]
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in mine + theirs):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ([os.environ.get("CXX", "g++")] + _cxx_flags() + ["-I", glm_dir, "-I", os.path.join(RAYZEN, "include"),
           "-I", os.path.join(_ROOT, "include"), "-shared", "-o", out] + [os.path.join(RAYZEN, f) for f in SOURCES] + [mine[0]])
    subprocess.check_call(cmd)
    return out


_libs = {}


def lib(path=None):
    path = path or LIBRARY
    if path not in _libs:
        if path == LIBRARY and not os.path.exists(path):
            build()
        L = C.CDLL(path)
        L.cppref_build_blas.restype = C.c_void_p
        L.cppref_build_blas.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.cppref_build_tlas.restype = C.c_void_p
        L.cppref_build_tlas.argtypes = [C.c_void_p, C.c_int]
        L.cppref_bvh_node_count.restype = C.c_size_t
        L.cppref_bvh_node_count.argtypes = [C.c_void_p]
        L.cppref_bvh_index_count.restype = C.c_size_t
        L.cppref_bvh_index_count.argtypes = [C.c_void_p]
        L.cppref_bvh_copy.restype = None
        L.cppref_bvh_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cppref_bvh_save.restype = C.c_int
        L.cppref_bvh_save.argtypes = [C.c_void_p, C.c_char_p]
        L.cppref_bvh_load.restype = C.c_void_p
        L.cppref_bvh_load.argtypes = [C.c_char_p]
        L.cppref_bvh_free.restype = None
        L.cppref_bvh_free.argtypes = [C.c_void_p]
        L.cppref_out_of_range_reads.restype = C.c_ulonglong
        L.cppref_out_of_range_reads.argtypes = []
        L.cppref_load_obj.restype = C.c_int
        L.cppref_load_obj.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int]
        _libs[path] = L
    return _libs[path]


def _take(L, h):
    nodes = np.zeros(L.cppref_bvh_node_count(h), NODE)
    idx = np.zeros(L.cppref_bvh_index_count(h), np.int32)
    L.cppref_bvh_copy(h, nodes.ctypes.data if nodes.size else None, idx.ctypes.data if idx.size else None)
    L.cppref_bvh_free(h)
    return nodes, idx


def _records(a, itemsize):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize != itemsize:
        raise TypeError(f"expected elements of {itemsize} bytes, got {a.dtype}")
    return a


def build_blas(triangles, method=SAH, library=None, want_axis_minus_one=False):
    """BVH::buildBLAS (BVH.cpp:99-175) -> (nodes, triIndices).  Finite vertices only: a NaN centroid breaks std::sort's
    ordering contract inside the reference.  want_axis_minus_one: also return how many vec3 reads of this build had an index
    outside 0..2 (BVH.cpp:140-144 after findSAHSplit found no split: axis == -1; the stand-in, like GLM 0.9.9.8 without
    asserts, reads x there)."""
    L = lib(library)
    t = _records(triangles, 64)
    before = L.cppref_out_of_range_reads()
    h = L.cppref_build_blas(t.ctypes.data if t.shape[0] else None, t.shape[0], int(method))
    if not h:
        raise RuntimeError("cppref_build_blas failed")
    out = _take(L, h)
    return out + (int(L.cppref_out_of_range_reads() - before),) if want_axis_minus_one else out


def build_tlas(roots, library=None):
    """BVH::buildTLAS (BVH.cpp:178-240) over world root boxes -> (nodes, triIndices).  At least one root: the reference loops
    for ever on none."""
    L = lib(library)
    r = _records(roots, 32)
    if r.shape[0] < 1:
        raise ValueError("BVH::buildTLAS does not terminate on zero instances")
    h = L.cppref_build_tlas(r.ctypes.data, r.shape[0])
    if not h:
        raise RuntimeError("cppref_build_tlas failed")
    return _take(L, h)


def load_obj(path, material_index, library=None):
    """Mesh::loadFromOBJ (Mesh.cpp:6-50) -> TRIANGLE records; pads and tail zero except where the reference wrote them."""
    L = lib(library)
    p = os.fsencode(path)
    n = L.cppref_load_obj(p, int(material_index), None, 0)
    if n == -1:
        raise FileNotFoundError(path)
    if n < 0:
        raise RuntimeError(f"the reference threw while reading {path}")
    tris = np.zeros(n, TRIANGLE)
    L.cppref_load_obj(p, int(material_index), tris.ctypes.data if n else None, n)
    return tris


def load_obj_text(text, material_index, library=None):
    """load_obj on `text` (bytes) written to a temporary file."""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "case.obj")
        with open(path, "wb") as f:
            f.write(text)
        return load_obj(path, material_index, library)


def save_load_round_trip(triangles, library=None):
    """buildBLAS, saveToFile, loadFromFile: -> ((nodes, idx) built, (nodes, idx) re-read, the file's bytes)."""
    L = lib(library)
    t = _records(triangles, 64)
    h = L.cppref_build_blas(t.ctypes.data if t.shape[0] else None, t.shape[0], SAH)
    if not h:
        raise RuntimeError("cppref_build_blas failed")
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "blas.bin")
        if L.cppref_bvh_save(h, os.fsencode(path)) != 0:
            raise OSError("BVH::saveToFile failed")
        raw = open(path, "rb").read()
        h2 = L.cppref_bvh_load(os.fsencode(path))
    if not h2:
        raise OSError("BVH::loadFromFile failed")
    return _take(L, h), _take(L, h2), raw
