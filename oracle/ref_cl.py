"""Recipe for oracle/_ref/libref_polygon2d.so: the reference's own contouring kernel, run on the CPU.

rendering/polygon2d.cl of the reference calls no generated evaluate(), so clang compiles it unmodified, as
OpenCL C, to an x86-64 object (cl_util/indexing.h force-included, as the reference's program assembly puts it
first).  oracle/ref_cl_shim.c supplies the six builtins the object leaves undefined and the loop over the work
items.  Nothing of the reference is copied: the library is built from the reference tree where there is one
(CODECAD_REFERENCE, default /root/reference) into oracle/_ref/, which git ignores; without the tree build()
does nothing and the tests run from tests/golden/polygon2d_ref.npz.

    python -m oracle.ref_cl            # build (both variants)
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
LIB_PATH = os.path.join(REF_DIR, "libref_polygon2d.so")
# the same recipe with contraction allowed and an fma dot: measures what the OpenCL specification leaves open
# (oracle/README.md); no test loads it
LIB_FMA_PATH = os.path.join(REF_DIR, "libref_polygon2d_fma.so")
_SHIM = os.path.join(_HERE, "ref_cl_shim.c")
_libs = {}

_f32p = ctypes.POINTER(ctypes.c_float)
_u32p = ctypes.POINTER(ctypes.c_uint32)


def reference_root():
    return os.environ.get("CODECAD_REFERENCE", "/root/reference")


def _sources():
    root = reference_root()
    return (os.path.join(root, "codecad", "rendering", "polygon2d.cl"), os.path.join(root, "codecad", "cl_util", "indexing.h"))


def find_clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (os.environ.get("CODECAD_CLANG"), os.path.join(rocm, "llvm", "bin", "clang"),
                 os.path.join(rocm, "lib", "llvm", "bin", "clang"), shutil.which("clang")):
        if cand and os.path.exists(cand):
            return cand
    return None


def _compile(clang, out, contract, shim_flags):
    kernel, header = _sources()
    obj = out[:-3] + ".kernel.o"
    target = ["-target", "x86_64-unknown-linux-gnu", "-fPIC", "-ffp-contract=" + contract] + (["-mfma"] if contract == "fast" else [])
    cmds = [[clang, "-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-O1"] + target
            + ["-include", header, "-c", kernel, "-o", obj],
            [clang, "-x", "c", "-std=gnu11", "-O1", "-Wall"] + target + shim_flags + ["-shared", "-o", out + ".tmp", _SHIM, "-x", "none", obj]]
    for cmd in cmds:
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError("building the reference kernel failed:\n%s\n%s" % (" ".join(cmd), proc.stderr[-4000:]))
    os.replace(out + ".tmp", out)
    os.remove(obj)


def build(force=False):
    """Build both libraries if the reference tree is there; -> LIB_PATH, or None where it is not."""
    src = _sources()
    if not all(os.path.exists(s) for s in src):
        return None
    outs = (LIB_PATH, LIB_FMA_PATH)
    deps = src + (_SHIM, os.path.abspath(__file__))
    if not force and all(os.path.exists(o) and all(os.path.getmtime(o) >= os.path.getmtime(d) for d in deps) for o in outs):
        return LIB_PATH
    clang = find_clang()
    if clang is None:
        raise RuntimeError("clang not found: cannot build oracle/_ref (set CODECAD_CLANG or ROCM_PATH)")
    os.makedirs(REF_DIR, exist_ok=True)
    _compile(clang, LIB_PATH, "off", [])
    _compile(clang, LIB_FMA_PATH, "fast", ["-DREF_FMA_DOT"])
    return LIB_PATH


def available():
    return os.path.exists(LIB_PATH)


def _lib(path):
    if path not in _libs:
        if not os.path.exists(path):
            raise RuntimeError("%s is not built: it is compiled from the reference tree (%s), which build() did not find; "
                               "the recorded results are in tests/golden/polygon2d_ref.npz"
                               % (os.path.relpath(path, os.path.dirname(_HERE)), reference_root()))
        lib = ctypes.CDLL(path)
        lib.ref_process_polygon.restype = ctypes.c_int
        lib.ref_process_polygon.argtypes = [_f32p, ctypes.c_float, _f32p, ctypes.c_uint32, ctypes.c_uint32, _f32p, _u32p, _u32p, _u32p]
        _libs[path] = lib
    return _libs[path]


def ref_process_polygon(corners, box_corner, box_step, fma=False):
    """The reference's process_polygon kernel itself over a float4 corner grid (gx, gy, 4): the same triple as
    oracle.process_polygon, (vertices float32 (cells, 2), links uint32 (cells,), starts uint32 (n,)) with the starts in
    launch order; vertices of empty cells are NaN (all bits set).  fma=True: the contracted build (measurements only)."""
    lib = _lib(LIB_FMA_PATH if fma else LIB_PATH)
    c = np.ascontiguousarray(corners, dtype=np.float32)
    gx, gy = int(c.shape[0]), int(c.shape[1])
    assert c.shape == (gx, gy, 4)
    cells = (gx - 1) * (gy - 1) * 2
    vertices = np.empty((cells, 2), dtype=np.float32)
    links = np.zeros(cells, dtype=np.uint32)
    starts = np.zeros(max((gx - 1) + (gy - 1), 1) * 2, dtype=np.uint32)
    count = ctypes.c_uint32(0)
    o = np.ascontiguousarray(np.asarray(box_corner, dtype=np.float64)[:2], dtype=np.float32)
    rc = lib.ref_process_polygon(o.ctypes.data_as(_f32p), ctypes.c_float(box_step), c.ctypes.data_as(_f32p), gx, gy,
                                 vertices.ctypes.data_as(_f32p), links.ctypes.data_as(_u32p), starts.ctypes.data_as(_u32p),
                                 ctypes.byref(count))
    if rc != 0:
        raise RuntimeError("ref_process_polygon failed with code %d" % rc)
    return vertices, links, starts[:count.value].copy()


if __name__ == "__main__":
    print(build(force=True) or "no reference tree at %s: nothing built" % reference_root())
