"""Mass properties of an assembly: volume, mass, centre of gravity and inertia per part and in total.

`assembly_mass_properties(asm, resolution, densities=None) -> AssemblyMassReport`.  The answer is defined on the lattice
of `interference()`, densely.

  * INSTANCES AND LATTICE.  Exactly those of `interference(asm, resolution)`: `_instance_cells.visible` and
    `checked_lattice`; sample (x, y, z) sits at `corner + step * (float)index` per axis in float32 (kernels.hpp sample()).
    One visible instance is enough; none gives an empty report.  ValueError as there: a 2D assembly, more than 64
    visible instances, a bad resolution, more than 65536 samples on an axis.
  * INSIDE.  Sample p is inside instance k when the tape of that instance alone gives w_k(p) < 0, strictly; a NaN is not
    inside.
  * TWO SAMPLE SETS PER INSTANCE.  V_k: the samples inside k -- the part on its own.  O_k: the samples inside k and
    inside no instance of lower index -- the part as the assembly owns it, by the lowest-index rule of `section()`'s
    `part_ids` and of the assembly picture's ids.  The O_k partition the samples inside the union, so a modelled overlap
    (a press fit, a pin through a planet) is counted once, for the lower index.
  * SUMS.  Each set has ten exact unsigned 64-bit index sums, in this order: n, x, y, z, xx, yy, zz, xy, xz, yz; V_k also
    has an index box (lo, hi).  Bit for bit they are what evaluating every instance over the whole lattice gives.
  * OVERFLOW.  ValueError when prod(dims) * (max(dims) - 1)^2 >= 2^64; below that no sum can overflow.
  * PHYSICAL QUANTITIES, on the host in float64 from the sums (`integrals`): a sample is a cube of side `step` centred on
    it; the ten integrals follow the convention of `mass_properties.integrals_host` -- centre moments plus step^2 / 12
    per cube on the diagonal second moments --, with the float32 `corner` and `step` widened to float64 as
    `_instance_cells.pair_fields` widens them; `mass_properties.finish()` turns integrals into a `MassProperties`.
  * DENSITIES.  None (every part 1.0), a sequence with one value per visible instance, or a dict from part name to
    density (a name that is missing gets 1.0; a name no visible instance has is ignored).  Every value finite and not
    negative, else ValueError.  The assembly's total is sum_k density_k * integrals(O_k) through `finish()`: its `volume`
    field is then a mass, its tensor a mass moment of inertia about the centre of gravity.

It is computed sparsely on the device, with one synchronisation, by the traversal under `interference()`
(_instance_cells.py) with one generalisation (csrc/instance_mass.hip): a cell of 4^k samples knows per instance not only
that it is still a candidate but also that it is FULL -- every sample of the cell inside.  A row has 32 bytes,
{x0 | y0 << 16, z0, cand lo, cand hi, full lo, full hi, 0, 0}, full a subset of cand; the host seeds the top level from the
instances' windows (every cell a window reaches, nothing full).  A level evaluates each candidate that is not yet full
at the centre of each child cell of s samples a side and, with thr = (s * step * sqrt(3) / 2) * (1 + 2^-10), the
threshold of `interference()`,
    w >= thr  drops the candidate,    w < -thr  makes it full,    anything else (a NaN too) leaves it a boundary candidate.
A child with no candidate is dropped; a child whose candidates are all full is RETIRED: each of them gets the closed-form
sums over the child's extents (clipped to dims) -- n = ex ey ez, the arithmetic series and the sums of squares -- and the
lowest of them gets the same as the owner; any other child goes on with both masks.  The finest level (4^3 samples)
evaluates the boundary candidates at every sample and takes the full ones as inside.  `retire=False` marks nothing
full: the same kernels, every cell descends to the finest level, the same sums -- the comparison arm.
`samples_evaluated` counts live lanes x candidates actually evaluated; inherited full candidates do not count.

PREMISE.  The traversal rests on what `k_classify` and `mass_properties()` already rest on: on BOTH sides of the surface
|w| does not exceed the distance to it (and the bounding box holds the instance).  Then w >= thr at a child's centre
proves every sample of the child outside and w < -thr every sample inside: the samples lie within (s - 1) step sqrt(3) / 2
of the centre, and thr leaves step sqrt(3) / 2 and 2^-10 of itself for the rounding of positions and of w.  Shapes from
`shapes.unsafe` break the premise, and so may any shape whose inner distance overshoots; then the sums may differ from
`retire=False`.
"""
import collections
import math

import numpy

from . import _instance_cells as cells
from . import util
from ._instance_cells import Instance
from .mass_properties import finish, _KEYS as _INTEGRALS

KEYS = ("n", "x", "y", "z", "xx", "yy", "zz", "xy", "xz", "yz")          # the order of the ten sums
_ACC = numpy.dtype([("v", "<u8", (10,)), ("o", "<u8", (10,)), ("lo", "<u4", (3,)), ("hi", "<u4", (3,)), ("pad", "<u4", (2,))])   # MassAcc
_ROW = 32


class PartMass(collections.namedtuple("PartMass", "index name density count volume mass properties index_box bounding_box "
                                                  "sums owned_sums")):
    """A visible instance on its own: `index` among the visible instances, `name`, `density`; over V_k, the samples
    inside it: `count`, `volume` = count * step^3, `mass` = density * volume, `properties` (a MassProperties at unit
    density), the min and max lattice index per axis (`index_box`) and the same in world coordinates (`bounding_box`;
    both None without a sample), the ten index `sums`; and `owned_sums`, the ten over O_k."""

    __slots__ = ()


class AssemblyMassReport(collections.namedtuple("AssemblyMassReport", "instances corner step dims parts total total_mass "
                                                                      "union_volume samples_evaluated traversals")):
    """`instances`, `corner`, `step`, `dims`: as in InterferenceReport; `parts`: a PartMass per visible instance;
    `total`: a MassProperties of the assembly weighted by density over the O_k (`volume` is the mass); `total_mass`;
    `union_volume` = sum_k n(O_k) * step^3; `samples_evaluated`: per-instance sample evaluations of the last traversal,
    on every level; `traversals`: how often it ran (more than once when a cell list overflowed; 0 for no instance)."""

    __slots__ = ()


def threshold(child, step):
    """float32 thr of a child cell of `child` samples a side: interference()'s."""
    return numpy.float32(child * float(step) * math.sqrt(3) / 2 * (1 + 2.0 ** -10))


def integrals(sums, corner, step):
    """The ten integrals {"1", "x", ..., "yz"} (mass_properties.finish's keys) over cubes of side `step` centred on the
    samples whose ten index sums are `sums`: the formulas of mass_properties.integrals_host with the sample itself as a
    cube's centre, in float64."""
    n, sx, sy, sz, sxx, syy, szz, sxy, sxz, syz = (float(v) for v in sums)
    s = float(step)
    cx, cy, cz = (float(c) for c in corner)
    s2 = s * s
    s3 = s * s2
    tx, ty, tz = s * sx, s * sy, s * sz
    return {
        "1": s3 * n,
        "x": s3 * (n * cx + tx), "y": s3 * (n * cy + ty), "z": s3 * (n * cz + tz),
        "xx": s3 * (n * (cx * cx + s2 / 12) + 2 * cx * tx + s2 * sxx),
        "yy": s3 * (n * (cy * cy + s2 / 12) + 2 * cy * ty + s2 * syy),
        "zz": s3 * (n * (cz * cz + s2 / 12) + 2 * cz * tz + s2 * szz),
        "xy": s3 * (n * cx * cy + cx * ty + cy * tx + s2 * sxy),
        "xz": s3 * (n * cx * cz + cx * tz + cz * tx + s2 * sxz),
        "yz": s3 * (n * cy * cz + cy * tz + cz * ty + s2 * syz),
    }


def part_densities(instances, densities):
    """[float] per visible instance from the `densities` argument (the module's docstring); ValueError for a sequence of
    another length or a value that is not a finite number >= 0."""
    if densities is None:
        values = [1.0] * len(instances)
    elif isinstance(densities, dict):
        values = [densities.get(i.name, 1.0) for i in instances]
        for v in densities.values():
            _checked_density(v)
    else:
        values = list(densities)
        if len(values) != len(instances):
            raise ValueError("densities has %d values, the assembly %d visible instances" % (len(values), len(instances)))
    return [_checked_density(v) for v in values]


def _checked_density(v):
    if isinstance(v, bool) or not isinstance(v, (int, float, numpy.floating, numpy.integer)) or not math.isfinite(v) or v < 0:
        raise ValueError("a density must be a finite number that is not negative, not %r" % (v,))
    return float(v)


def check_overflow(dims):
    """ValueError when a second-moment index sum over the whole lattice could reach 2^64."""
    d = [int(v) for v in dims]
    if d[0] * d[1] * d[2] * (max(d) - 1) ** 2 >= 2 ** 64:
        raise ValueError("a lattice of %s samples: its index sums could overflow 64 bits; use a coarser resolution" % (d,))


def top_rows(instances, corner, step, dims, side):
    """uint32[n, 8] rows of the top level: every cell of `side` samples that a window reaches, nothing full."""
    rows = cells.cell_rows(cells.windows(instances, corner, float(step), dims), dims, side, least=1)
    return numpy.hstack([rows, numpy.zeros_like(rows)])


def report(instances, corner, step, dims, acc, rho, evaluations, traversals):
    """The AssemblyMassReport of the accumulators `acc` (_ACC, one per instance)."""
    c64, s64 = corner.astype(numpy.float64), float(step)
    cell = s64 ** 3
    parts = []
    total = dict.fromkeys(_INTEGRALS, 0.0)
    owned = 0
    for k, (inst, a) in enumerate(zip(instances, acc)):
        sums, owned_sums = tuple(int(v) for v in a["v"]), tuple(int(v) for v in a["o"])
        index_box = box = None
        if sums[0]:
            lo, hi = tuple(int(v) for v in a["lo"]), tuple(int(v) for v in a["hi"])
            index_box = (lo, hi)
            box = util.BoundingBox(cells.index_position(corner, step, lo), cells.index_position(corner, step, hi))
        parts.append(PartMass(k, inst.name, rho[k], sums[0], sums[0] * cell, rho[k] * sums[0] * cell,
                              finish(integrals(sums, c64, s64)), index_box, box, sums, owned_sums))
        for key, value in integrals(owned_sums, c64, s64).items():
            total[key] += rho[k] * value
        owned += owned_sums[0]
    return AssemblyMassReport([Instance(i.name, i) for i in instances], corner, step, dims, parts, finish(total),
                              total["1"], owned * cell, evaluations, traversals)


def assembly_mass_properties(asm, resolution, densities=None, initial_capacity=None, retire=True):
    """Mass properties of the visible instances of the 3D assembly `asm` on the lattice of `interference(asm, resolution)`,
    each on its own and all together with every overlap counted once (the module's docstring defines the sample sets, the
    sums, the physical quantities and what the traversal assumes) -> AssemblyMassReport.

    `densities`: None, one value per visible instance, or {part name: density}.  `retire=False` retires no cell: every
    boundary and interior sample is evaluated at the finest level (the same sums, slower).  `initial_capacity` caps the
    first guess of every cell list, as in interference().  Raises ValueError for what interference() refuses, for a bad
    density and for a lattice whose index sums could overflow 64 bits."""
    instances = cells.visible(asm, resolution)
    corner, step, dims = cells.checked_lattice(instances, resolution)
    rho = part_densities(instances, densities)
    check_overflow(dims)
    n = len(instances)
    empty = numpy.zeros(n, dtype=_ACC)
    if n == 0:
        return report(instances, corner, step, dims, empty, rho, 0, 0)
    side = cells.top_side(dims)
    top = top_rows(instances, corner, step, dims, side)
    if len(top) == 0:
        return report(instances, corner, step, dims, empty, rho, 0, 0)
    evaluations, acc, traversals = cells.traverse(
        instances, top, side, corner, step, dims, initial_capacity, pair_dtype=_ACC, pair_init={"lo": 0xffffffff},
        thr=lambda child: threshold(child, step), cells="hu_assembly_mass_cells", finest=[("hu_assembly_mass_leaf", ())],
        row_bytes=_ROW, cells_extra=(int(bool(retire)),), accumulators=n)
    return report(instances, corner, step, dims, acc, rho, evaluations, traversals)
