"""What a 3-axis cutter along a lattice axis cannot reach: the material of the part-id volume of an assembly that the design
wants gone and that the cutter, with the spindle along the axis, cannot remove -- what is hidden under something, and what is
in plain view but too narrow for the tool: inside corners, slots narrower than the tool, the fillet a ball nose leaves at the
foot of a wall.  Its by-product is the drop-cutter surface, the lowest tip position over every column: the raster toolpath.

`tool_access(asm, resolution, axis=2, up=True, tool=flat_tool(1), of=SOLID) -> ToolAccessReport`.  Everything is defined on
the index space Z^3 of the lattice of `assembly_voxels(asm, resolution)`, in integers, exact, and independent of the order in
which anything ran.

  * INSTANCES, LATTICE, PART_IDS, `of`, `axis`, `up`.  Exactly those of `overhangs()`, through the same helpers: the same
    ValueErrors, the same `retire=True` traversal, the same bytes.  S is the samples with part_ids != 255 (`of=SOLID`) or with
    part_ids == k (`of=k`: the samples of every other part count as empty).  The LAYER of p is h(p) = p[axis] if `up`, else
    n_a - 1 - p[axis].  The table (plate, vice) lies under layer 0; the spindle is beyond layer n_a - 1 and points at the table.
    Nothing outside the lattice is in S, and the padding z in [nz, pz) of the device buffers is never read as data.
  * COLUMNS.  (u, v) are the two axes other than `axis`, in increasing order: axis 0 gives (y, z), axis 1 (x, z), axis 2
    (x, y).  A 2D field is [nu][nv], v fastest.
  * TOOL.  `Tool(radius_sq, profile)`: `radius_sq` an integer 0..1024 (MAX_RADIUS_SQ), K = isqrt(radius_sq) <= 32;
    `profile[d2]`, d2 = 0..radius_sq, integers 0..65535, non-decreasing from profile[0] = 0: how far above the tip the tool's
    underside lies at the squared lateral distance d2 (ValueError otherwise).  D is the offsets n = (du, dv) with
    du^2 + dv^2 <= radius_sq and g(n) = profile[du^2 + dv^2].  `flat_tool(radius_sq)` is an end mill, all zeros;
    `ball_tool(k)` has radius_sq = k^2 and profile[d2] = k - isqrt(k^2 - d2).  Lengths are lattice steps, as `reach_sq` is.
  * TOPS.  T(c) = 1 + the greatest layer of a sample of S on column c, 0 when the column holds none; top_id(c) is the
    part_ids byte of that sample, 255 when there is none.  Outside the lattice T = 0.
  * TIPS.  Z, the drop-cutter surface, on the PADDED DOMAIN -K <= u < nu + K, -K <= v < nv + K: Z(c) = the greatest
    T(c + n) - g(n) over n in D (n = 0 gives T(c) >= 0: no clamp).  With its tip at height Z(c) over c the tool touches S and
    enters it nowhere.
  * CUT.  On the lattice's columns C(c) = the least Z(c - n) + g(n) over n in D: the closing of T by the tool.  Every sample
    of column c in a layer >= C(c) is swept by the tool somewhere, none below C(c) is.  C >= T.
  * CROWD.  crowd(c) = the top_id of the column with the greatest T among c + n, n in D, inside the lattice, ties to the
    lowest id; 255 when all those T are 0.  Where C(c) > T(c) that T is greater than T(c): the wall that keeps the tool out.
  * REST.  The samples of the lattice not in S in a layer h < C(column), of two disjoint kinds: UNDERCUT, h < T(c), with the
    id of its HOLDER, the nearest sample of S above it on its line (as `overhangs` defines a holder); TIGHT,
    T(c) <= h < C(c), with the id crowd(c).  `rest_ids`, uint8[nx, ny, nz] in the format of `part_ids`: the id on REST, 255
    elsewhere; `tops` tells the kinds apart (`undercut_mask()`, `tight_mask()`).
  * PER PART, counted on the device in uint64, Python ints here.  `undercut_counts[k]`: the undercut samples whose holder is
    k; `tight_counts[k]`: the tight samples whose crowding part is k; `counts[k]`: as in AssemblyVoxels.
  * POCKETS.  `pockets`: the 6-connected components of REST as `Component`s of `assembly_components`, found by that module's
    kernels over `rest_ids`; `labels`, uint32[nx, ny, nz]: a pocket's label at its samples, NONE elsewhere.
  * FIELDS.  `tops[nu, nv]`, `tips[nu + 2K, nv + 2K]` with its origin at (-K, -K), `cut[nu, nv]`: numpy int32;
    `crowd[nu, nv]`: uint8.
No visible instance (or no top row) launches nothing: `tops`, `cut` and `tips` all zeros, `crowd` and `rest_ids` all 255,
`labels` all NONE, no pocket.

WHAT FOLLOWS.  Z >= T on the lattice.  `flat_tool(0)` gives Z = T = C there and no tight sample, and its UNDERCUT from the
first layer h0 of `overhangs()` up is the support set of `overhangs(reach_sq=0)`.  IDEMPOTENCE: S with REST added has no rest
under the same tool, and its T is C.  The REST of `flat_tool(a)` is within that of `flat_tool(b)` where the disc of b is a union
of translates of the disc of a (every b for a = 0; not the 3 x 3 square of radius_sq 2 for the plus sign of radius_sq 1).

ON THE DEVICE (csrc/instance_tool.hip), four launches on one stream, no host wait between them.  `hu_tool_tops` scans the
volume from the spindle side down into a field of keys T * 256 + (255 - top_id); `hu_tool_dilate` and `hu_tool_erode` are the
2D stage: a workgroup stages a tile of 32 x 32 columns and a halo of K in LDS, and the profile, and every lane takes the
maximum of T - g (the minimum of Z + g, then the greatest key: the crowd) over the up to 3209 offsets of D from LDS;
`hu_tool_rest` walks every line from the spindle side down once more with the holder carried -- per lane in a register along
x and y, through the ballots of a word with a carry from word to word along z -- and writes `rest_ids` and the counts.
DEVICE MEMORY.  While the kernels run the ids and `rest_ids` are held, 2 bytes a sample of the device buffer nx * ny * pz,
and the 2D fields, 4 (2 nu nv + (nu + 2K)(nv + 2K)) bytes; the labelling afterwards holds `rest_ids` and the labels, 5 bytes
a sample: the peak.  ValueError when 5 * nx * ny * pz plus the fields exceeds max_bytes, and when the label volume would have
more than 2^31 entries, before anything is launched.
OUT OF SCOPE here: spindle directions off the lattice axes, tool holders and shanks wider than the cutter, stock other than
the lattice box, combining several setups, toolpaths in world coordinates, more than 64 instances, several devices.
"""
import collections
import math

import numpy

from . import _instance_cells as cells
from . import hip_util
from .assembly_voxels import _device_volume, _whole, _of_code, _axis, _dims, _cropped, _LabelMask, EMPTY
from .assembly_components import SOLID, NONE, _components, _label_volume, _check_entries
from .hip_util import manager as hip_manager, check

MAX_RADIUS_SQ = 1024            # include/hip_util.h HU_TOOL_MAX_RADIUS_SQ
TILE = 32                       # HU_TOOL_TILE: the columns of a workgroup of the 2D stage, a side
SAMPLE_BYTES = 5                # rest_ids and the labels: what is held per sample at the peak
_ACC = (2, 64)                  # uint64: UNDERCUT per holder, TIGHT per crowding part


class Tool(collections.namedtuple("Tool", "radius_sq profile")):
    """A cutter: `radius_sq`, the squared radius in lattice steps, and `profile`, a tuple of radius_sq + 1 heights of its
    underside above its tip, by squared lateral distance (the module's docstring).  ValueError for anything else."""
    __slots__ = ()

    def __new__(cls, radius_sq, profile):
        if not _whole(radius_sq, 0, MAX_RADIUS_SQ):
            raise ValueError("radius_sq must be an integer from 0 to %d, not %r" % (MAX_RADIUS_SQ, radius_sq))
        try:
            profile = tuple(profile)
        except TypeError:
            raise ValueError("profile must be a sequence of radius_sq + 1 integers, not %r" % (profile,))
        if len(profile) != radius_sq + 1 or not all(_whole(g, 0, 65535) for g in profile):
            raise ValueError("profile must hold radius_sq + 1 = %d integers from 0 to 65535" % (radius_sq + 1))
        if profile[0] != 0 or any(b < a for a, b in zip(profile, profile[1:])):
            raise ValueError("profile must start at 0 and never decrease")
        return super().__new__(cls, int(radius_sq), tuple(int(g) for g in profile))

    @property
    def reach(self):
        """K = isqrt(radius_sq): how many columns the tool reaches to a side."""
        return math.isqrt(self.radius_sq)


def flat_tool(radius_sq):
    """An end mill of squared radius `radius_sq`: a flat underside."""
    if not _whole(radius_sq, 0, MAX_RADIUS_SQ):
        raise ValueError("radius_sq must be an integer from 0 to %d, not %r" % (MAX_RADIUS_SQ, radius_sq))
    return Tool(radius_sq, (0,) * (int(radius_sq) + 1))


def ball_tool(k):
    """A ball nose of radius `k` lattice steps, 0..32: profile[d2] = k - isqrt(k^2 - d2)."""
    if not _whole(k, 0, math.isqrt(MAX_RADIUS_SQ)):
        raise ValueError("the radius of a ball must be an integer from 0 to %d, not %r" % (math.isqrt(MAX_RADIUS_SQ), k))
    k = int(k)
    return Tool(k * k, tuple(k - math.isqrt(k * k - d2) for d2 in range(k * k + 1)))


class ToolAccessReport(_LabelMask, collections.namedtuple("ToolAccessReport", "instances corner step dims of axis up tool part_ids tops tips cut "
                                                                  "crowd rest_ids counts undercut_counts tight_counts pockets labels "
                                                                  "samples_evaluated traversals component_capacity_runs")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `counts`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    `component_capacity_runs`: as in ComponentsReport; every other field: the module's docstring."""
    __slots__ = ()

    def rest_volume(self):
        """|REST| * step^3: the material the cutter leaves."""
        return (sum(self.undercut_counts) + sum(self.tight_counts)) * float(self.step) ** 3

    @property
    def machinable(self):
        """The cutter leaves nothing: there is no rest."""
        return sum(self.undercut_counts) + sum(self.tight_counts) == 0

    def _layers_and_tops(self):
        shape = self.rest_ids.shape
        along = numpy.indices(shape)[self.axis]
        return along if self.up else shape[self.axis] - 1 - along, numpy.expand_dims(self.tops, self.axis)

    def undercut_mask(self):
        """bool[nx, ny, nz]: the rest under a top of its column."""
        h, tops = self._layers_and_tops()
        return (self.rest_ids != EMPTY) & (h < tops)

    def tight_mask(self):
        """bool[nx, ny, nz]: the rest in view of the spindle that the tool is too wide for."""
        h, tops = self._layers_and_tops()
        return (self.rest_ids != EMPTY) & (h >= tops)


def field_shape(shape, axis):
    """(nu, nv): the columns of a lattice of `shape` seen along `axis`."""
    return tuple(int(shape[a]) for a in range(3) if a != axis)


def tool_access(asm, resolution, axis=2, up=True, tool=flat_tool(1), of=SOLID, initial_components=None, initial_capacity=None,
                max_bytes=2 ** 32):
    """The material around the visible instances of the 3D assembly `asm`, on the lattice of `interference(asm, resolution)`,
    that the cutter `tool` with the spindle along lattice axis `axis` (above the last layer, or above the first with
    `up=False`) cannot remove, and the drop-cutter surface (the module's docstring defines them) -> ToolAccessReport.

    `tool`: a Tool (`flat_tool`, `ball_tool`).  `of`: SOLID, or the index of a visible instance.  `initial_components` caps
    the first guess of the pocket table, `initial_capacity` that of every cell list of the voxel traversal.  Raises ValueError
    for what assembly_voxels() refuses, for a bad `of`, `axis` or `tool`, more than 2^31 label entries and for volumes and
    fields of more than `max_bytes` bytes together."""
    n = len(cells.visible(asm, resolution))
    code, axis = _of_code(of, n), _axis(axis)
    if not isinstance(tool, Tool):
        raise ValueError("tool must be a Tool (flat_tool(radius_sq), ball_tool(k)), not %r" % (tool,))
    up, K = bool(up), tool.reach

    def fields_fit(dims):
        _check_entries(dims)
        nx, ny, nz = (int(d) for d in dims)
        nu, nv = field_shape(dims, axis)
        needed = SAMPLE_BYTES * nx * ny * (-(-nz // 16) * 16) + 4 * (2 * nu * nv + (nu + 2 * K) * (nv + 2 * K))
        if needed > max_bytes:
            raise ValueError("a lattice of %s samples and its fields need %d bytes, more than max_bytes = %d; use a coarser resolution"
                             % ([nx, ny, nz], needed, max_bytes))

    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=SAMPLE_BYTES, check_dims=fields_fit)
    shape = tuple(int(d) for d in voxels.dims)
    nu, nv = field_shape(shape, axis)
    pu, pv = nu + 2 * K, nv + 2 * K

    def report(tops, tips, cut, crowd, rest, totals, pockets, labels, runs):
        return ToolAccessReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, of, axis, up, tool, voxels.part_ids, tops, tips,
                                cut, crowd, rest, voxels.counts, totals[0], totals[1], pockets, labels, voxels.samples_evaluated,
                                voxels.traversals, runs)

    if volume is None:
        return report(numpy.zeros((nu, nv), numpy.int32), numpy.zeros((pu, pv), numpy.int32), numpy.zeros((nu, nv), numpy.int32),
                      numpy.full((nu, nv), EMPTY, numpy.uint8), numpy.full(shape, EMPTY, numpy.uint8), [[0] * n for _ in range(2)], [],
                      numpy.full(shape, NONE, numpy.uint32), 0)
    lib, queue = hip_manager.lib, hip_manager.queue
    nx, ny, pz = volume.shape
    dims = _dims(shape)
    acc = hip_util.Buffer(numpy.uint64, _ACC, queue=queue)
    check(lib.hu_memset(acc.device_ptr, 0, acc.size, queue.handle), "hu_memset")
    profile = hip_util.Buffer(numpy.uint16, (tool.radius_sq + 1,), queue=queue)
    profile.enqueue_write(numpy.array(tool.profile, dtype=numpy.uint16))
    fields = hip_util.Buffer(numpy.uint32, (2 * nu * nv + pu * pv,), queue=queue)       # the tops, the cut, the tips
    tops, cut, tips = fields.device_ptr, fields.device_ptr + 4 * nu * nv, fields.device_ptr + 8 * nu * nv
    rest = hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue)
    check(lib.hu_tool_tops(volume.device_ptr, tops, dims, pz, axis, int(up), code, queue.handle), "hu_tool_tops")
    check(lib.hu_tool_dilate(tops, profile.device_ptr, tips, nu, nv, tool.radius_sq, queue.handle), "hu_tool_dilate")
    check(lib.hu_tool_erode(tips, tops, profile.device_ptr, cut, nu, nv, tool.radius_sq, queue.handle), "hu_tool_erode")
    check(lib.hu_tool_rest(volume.device_ptr, tops, cut, rest.device_ptr, acc.device_ptr, dims, pz, axis, int(up), code, queue.handle),
          "hu_tool_rest")
    rest_ids = _cropped(rest, shape[2])
    words = fields.read()
    totals = acc.read()
    for b in (volume, fields, profile, acc):
        b.release()
    labels, rows, runs = _label_volume(rest, shape, 1, True, initial_components)
    keys, closed = words[:nu * nv].reshape(nu, nv), words[nu * nv:2 * nu * nv].reshape(nu, nv)
    return report((keys >> 8).astype(numpy.int32), words[2 * nu * nv:].reshape(pu, pv).astype(numpy.int32), (closed >> 8).astype(numpy.int32),
                  (closed & 255).astype(numpy.uint8), rest_ids, [[int(v) for v in totals[k, :n]] for k in range(2)],
                  _components(rows, voxels.corner, voxels.step), labels, runs)
