"""The order in which the dense float4 grid hands its 16^3 boxes to workgroups (csrc/kernels.hpp grid_eval_boxes: the box
list in chunks of 256, inside a chunk a contiguous eighth per XCD) changes WHICH workgroup evaluates which box and nothing
else: every voxel of `hu_grid_eval_slab`'s float4 grid equals `oracle.evaluate_points` at its sample point bit for bit
(-0 != +0, NaN = NaN).  Only per-tape code with deferred directions goes over boxes and so through the new order (both
tapes here: several primitives, no rounded blends); the interpreter evaluates runs along z and is held to the same
figures as the second evaluator of the same grids.  Shapes: the smallest at which the order can go wrong -- one box; fewer
boxes than XCDs; 9 boxes (q = 1, r = 1 in the split of a chunk); 5 boxes along x and along y; 64 boxes; 288 boxes (one whole
chunk and a partial one of 32); a slab that starts inside the grid; 20 x 12 x 24, whose rim boxes are partial but whose
extents are multiples of (4, 4, 8): k_grid_eval; and extents that are no such multiples, which take k_grid_eval_ragged:
4 boxes, and 294 boxes (a whole chunk and one of 38)."""
import ctypes

import numpy as np
import pytest

import oracle
from conftest import same_bits

pytestmark = pytest.mark.gpu

# (dims, x0, planes)
CASES = [
    ((16, 16, 16), 0, 16),
    ((32, 16, 48), 0, 32),
    ((48, 48, 16), 0, 48),
    ((80, 16, 16), 0, 80),
    ((16, 80, 16), 0, 16),
    ((64, 64, 64), 0, 64),
    ((64, 64, 64), 16, 32),
    ((32, 96, 96), 0, 32),      # 2 x 6 x 6 x 4 = 288 boxes: more than one chunk of 256
    ((20, 12, 24), 0, 20),      # partial boxes at the rim, whole bricks: still k_grid_eval
    ((21, 13, 25), 0, 21),      # no multiples of (4, 4, 8): k_grid_eval_ragged, 2 x 1 x 2 boxes
    ((20, 12, 20), 0, 20),      # ragged along z only
    ((82, 98, 100), 0, 82),     # k_grid_eval_ragged, 6 x 7 x 7 = 294 boxes: more than one chunk
    ((82, 98, 100), 13, 37),    # ... and a ragged slab of it that starts inside a box
]
_wanted = {}


def tapes():
    from codecad_amd import examples, nodes
    return {"sponge2": (examples.sponge(2), nodes.make_program(examples.sponge(2))),
            "csg_example": (examples.csg_example(), nodes.make_program(examples.csg_example()))}


def grid_of(shape, dims):
    bb = shape.bounding_box()
    extent = max(bb.b.x - bb.a.x, bb.b.y - bb.a.y, bb.b.z - bb.a.z)
    step = np.float32(extent / max(dims))
    corner = np.array([bb.a.x + extent / max(dims) / 2, bb.a.y + extent / max(dims) / 2, bb.a.z + extent / max(dims) / 2], np.float32)
    return corner, step


def wanted(name, shape, tape, dims):
    """oracle.evaluate_points at the kernels' sample points (corner + step * index, in binary32), once per tape and grid"""
    key = (name, dims)
    if key not in _wanted:
        corner, step = grid_of(shape, dims)
        axes = [corner[a] + step * np.arange(dims[a], dtype=np.float32) for a in range(3)]
        assert all(a.dtype == np.float32 for a in axes)
        pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
        _wanted[key] = oracle.evaluate_points(tape, pts).reshape(dims + (4,))
        _wanted[key].setflags(write=False)
    return _wanted[key]


@pytest.mark.parametrize("evaluator", ["specialised", "interpreter"])
@pytest.mark.parametrize("name", ["sponge2", "csg_example"])
def test_dense_float4_grid_equals_the_oracle_on_every_voxel(hip, name, evaluator):
    import torch
    from codecad_amd import hip_util
    from codecad_amd.hip_util import check
    shape, tape = tapes()[name]
    handle = hip_util.Tape(tape)
    if evaluator == "specialised":
        handle.specialize(hip_util.SPEC_DENSE)
        assert handle.groups & hip_util.SPEC_DENSE == hip_util.SPEC_DENSE, "the dense kernels' per-tape code is not loaded"
    fptr = ctypes.POINTER(ctypes.c_float)
    for dims, x0, count in CASES:
        corner, step = grid_of(shape, dims)
        c4 = np.zeros(4, np.float32)
        c4[:3] = corner
        d = (ctypes.c_uint32 * 3)(*dims)
        slab = torch.full((count, dims[1], dims[2], 4), float("nan"), dtype=torch.float32, device="cuda")
        check(hip.lib.hu_grid_eval_slab(handle.device_ptr, c4.ctypes.data_as(fptr), step, d, x0, count, 0, slab.data_ptr(), None), "slab")
        torch.cuda.synchronize()
        got = slab.cpu().numpy()
        want = wanted(name, shape, tape, dims)[x0:x0 + count]
        bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
        assert same_bits(got, want), "%s, %s, grid %s, planes %d..%d: %d floats differ, the first at voxel %s" % (
            name, evaluator, dims, x0, x0 + count, int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0][:3]))
    handle.release()
