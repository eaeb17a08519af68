"""The parts of an assembly as binary STL files, one per visible instance, as placed (codecad_amd/assembly_meshes.py): the
welded mesh of every instance, all on one lattice, so that parts line up sample for sample.  The 50-byte records are those
of stl_renderer.RECORD, built with NumPy on the host from the welded mesh: float32 corners, the unnormalised float32 cross
product (v1 - v0) x (v2 - v0) as the normal, attribute 0."""
import os
import re

import numpy

from ..assembly_meshes import assembly_meshes
from .stl_renderer import RECORD, write_stl


def stl_records(vertices, triangles):
    """One RECORD per triangle of an indexed mesh, on the host."""
    vertices = numpy.asarray(vertices, dtype=numpy.float64).reshape(-1, 3)
    triangles = numpy.asarray(triangles, dtype=numpy.int64).reshape(-1, 3)
    records = numpy.zeros(len(triangles), dtype=RECORD)
    records["vectors"] = vertices[triangles].astype(numpy.float32)
    v = records["vectors"]
    records["normal"] = numpy.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return records


def stl_name(k, name):
    """The file of instance k: its index and its name, characters outside [A-Za-z0-9._-] replaced by `_`."""
    return "%02d_%s.stl" % (k, re.sub(r"[^A-Za-z0-9._-]", "_", str(name)))


def write_assembly_stl(meshes, directory):
    """Writes every instance of a Meshes as `directory`/stl_name(k, name) (the directory is made) -> the list of paths."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for k, inst in enumerate(meshes.instances):
        path = os.path.join(directory, stl_name(k, inst.name))
        write_stl(path, stl_records(*meshes.mesh(k)))
        paths.append(path)
    return paths


def render_assembly_stl(asm, directory, resolution=None):
    """Meshes the visible instances of the 3D assembly `asm` at `resolution` (default: half the feature size of its
    shape, as mesh_arrays takes it) and writes one binary STL per instance into `directory` -> the list of paths.  Raises
    the ValueErrors of assembly_meshes()."""
    if resolution is None:
        resolution = asm.shape().feature_size() / 2
    return write_assembly_stl(assembly_meshes(asm, resolution), directory)
