"""Where a caller may put the part-id volume and what goes with it: ANY pitch that is a multiple of 16 from nz to 65536, and every
pointer at no more than the alignment its entry point states (include/hip_util.h; the entry points' checks are the contract).
test_gpu_pitch_alignment.py runs the id-volume entry points over buffers placed by this module, test_pitch_alignment_host.py
proves on the CPU that the placements and the cases hold the edges they are named for.  Plain numpy and hip_util.Buffer.

A PLACEMENT is a pitch rule and a rule for a buffer's device address, given the alignment `a` its entry point asks for:
  tight    pitch = ceil16(nz), the address a multiple of 256: what the rest of the suite does, the control;
  word     pitch = ceil16(nz) + 16, the least legal pitch that is not the tight one; address % (2 a) == a: aligned to a and to
           no more (a = 1: an odd address);
  segment  pitch = ceil64(nz) + 64 + 16: a whole 64-sample segment of every column is padding, the pitch is no multiple of 64
           and pitch / 64 > ceil(nz / 64); the addresses as for `word`.
A PLACED buffer is an oversized uint8 allocation: at least GUARD bytes of SENTINEL, the array, at least GUARD bytes of SENTINEL.
Inputs carry the per-consumer POISON of raw_volume_scenes.py over their whole padding [nz, pitch); outputs are SENTINEL all
over.  Placed.read gives the lattice's part, the padding and the two guards apart.

THE CASES are the smallest raw cases the suite has that between them hold nz % 16 != 0, nz > 64 and nz % 64 == 0 per family,
with their references, which take raw ids and know nothing of a pitch.  A family's ARMS are the calls made per case: the
directions, the `local` arms, the transforms.  reference(family, case, arm) is an ordered dict name -> (kind, value):
  "volume"  [..][nz] last, compared on the lattice;  "table"  counts, keys, rows, words: compared whole;
  "labels"  linear indices, which depend on the lattice's nz (the device's are buffer indices until they are converted);
  "field"   a 2D field of the tool kernels whose extent follows nz along the walks over x and y;
  "far"     the farthest samples of hu_geodesic_stats as (d + 1, x, y, z): the device's key holds a buffer index, which the test
            converts with the placed pitch.
reference(..., widen=pitch) is the same reference over the volume AS IF ITS PADDING WERE DATA, the lattice nz' = pitch: the host
test asserts that it differs, so a kernel that read the padding would not pass.  BLIND arms are those whose padding columns are
independent of the lattice's and feed no count (the thickness passes along x and y with finish == 0): there the widened reference
EQUALS the true one on the lattice, which the host test asserts instead; their stride and bounds are still exercised."""
import collections
import functools
import math

import numpy

import raw_volume_scenes as raw
import thin_walls_scenes as thin
import disassembly_scenes as dis
import overhangs_scenes as over
import assembly_components_scenes as comp
import contacts_scenes as con
import drainage_scenes as drain
import islands_scenes as isl
import tool_access_scenes as tool
import wall_thickness_scenes as wall
import flow_length_scenes as flow
from raw_volume_scenes import SOLID, EMPTY, NONE, ceil16

GUARD = 256                     # bytes of sentinel on either side of a placed array, at the least
SENTINEL = 0xa5

Placement = collections.namedtuple("Placement", "name pitch_of minimal")
PLACEMENTS = collections.OrderedDict((p.name, p) for p in (
    Placement("tight", ceil16, False),
    Placement("word", lambda nz: ceil16(nz) + 16, True),
    Placement("segment", lambda nz: -(-int(nz) // 64) * 64 + 64 + 16, True)))


def address(base, align, placement):
    """The device address of an array of alignment `align` in an allocation that starts at `base`."""
    first = int(base) + GUARD
    if not placement.minimal:
        return -(-first // 256) * 256
    return -(-first // (2 * align)) * (2 * align) + align


def slack(align):
    """The bytes an allocation holds beyond the array: both guards, and room for address()."""
    return 2 * GUARD + 256 + 2 * align


def sentinel(dtype, shape):
    """An array whose every byte is SENTINEL."""
    return numpy.full(int(numpy.prod(shape)) * numpy.dtype(dtype).itemsize, SENTINEL, dtype=numpy.uint8).view(dtype).reshape(shape)


class Placed:
    """`host` on the device at address(...) of an allocation of its own.  nz: the lattice's extent along the last axis, where
    the array is a pitched volume."""

    def __init__(self, queue, host, align, placement, nz=None):
        from codecad_amd import hip_util
        host = numpy.ascontiguousarray(host)
        self.dtype, self.shape, self.nbytes, self.nz, self.align = host.dtype, host.shape, host.nbytes, nz, align
        self.buffer = hip_util.Buffer(numpy.uint8, (host.nbytes + slack(align),), queue=queue)
        base = self.buffer.device_ptr
        self.ptr = address(base, align, placement)
        self.offset = self.ptr - base
        if placement.minimal:
            assert self.ptr % (2 * align) == align, (hex(self.ptr), align)
        else:
            assert self.ptr % 256 == 0
        assert self.offset >= GUARD and self.buffer.size - self.offset - self.nbytes >= GUARD
        image = numpy.full(self.buffer.size, SENTINEL, dtype=numpy.uint8)
        image[self.offset:self.offset + self.nbytes] = host.reshape(-1).view(numpy.uint8)
        self.buffer.enqueue_write(image)

    def at(self, byte_offset):
        return self.ptr + byte_offset

    def read(self):
        """(the lattice's part, the padding, (the guard before, the guard after)); a buffer that is no volume is all lattice."""
        image = self.buffer.read().copy()
        body = image[self.offset:self.offset + self.nbytes].copy().view(self.dtype).reshape(self.shape)
        guards = (image[:self.offset], image[self.offset + self.nbytes:])
        if self.nz is None:
            return body, body.reshape(-1)[:0], guards
        return body[..., :self.nz], body[..., self.nz:], guards

    def refill(self, host):
        """The array again (an output between two arms); the guards are left as they are."""
        from codecad_amd.hip_util import check
        host = numpy.ascontiguousarray(host)
        assert host.nbytes == self.nbytes
        lib, queue = self.buffer.manager.lib, self.buffer.queue
        check(lib.hu_memcpy_h2d(self.ptr, host.ctypes.data, host.nbytes, queue.handle), "hu_memcpy_h2d")
        queue.synchronize()

    def release(self):
        self.buffer.release()


def mismatches(got, want, limit=8):
    """The first `limit` (index, got, want) of two arrays or lists that should be EQUAL; a shape that differs is one too."""
    if isinstance(want, numpy.ndarray) or isinstance(got, numpy.ndarray):
        got, want = numpy.asarray(got), numpy.asarray(want)
        if got.shape != want.shape:
            return [("shape", got.shape, want.shape)]
        if got.dtype.kind in "iub" and want.dtype.kind in "iub":                  # (uint64 against int64: compare as Python would)
            got, want = got.astype(object) if got.dtype != want.dtype else got, want.astype(object) if got.dtype != want.dtype else want
        wrong = numpy.argwhere(got != want)
        return [(tuple(int(v) for v in k), got[tuple(k)].item() if hasattr(got[tuple(k)], "item") else got[tuple(k)],
                 want[tuple(k)].item() if hasattr(want[tuple(k)], "item") else want[tuple(k)]) for k in wrong[:limit]]
    got, want = list(got), list(want)
    if len(got) != len(want):
        return [("length", len(got), len(want))]
    return [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:limit]


# ---- labels: buffer indices and linear indices --------------------------------------------------------------------------

def buffer_index(linear, nz, pitch):
    """The index into a label buffer of pitch `pitch` of the linear index (x * ny + y) * nz + z; NONE stays."""
    q = linear.astype(numpy.int64)
    return numpy.where(linear == NONE, NONE, q + (q // nz) * (pitch - nz)).astype(numpy.uint32)


def linear_index(entries, nz, pitch):
    """The conversion back, as hu_components_finish and the tests' linear_of make it."""
    q = entries.astype(numpy.int64)
    return numpy.where(entries == NONE, NONE, q - (q // pitch) * (pitch - nz)).astype(numpy.uint32)


# ---- the cases ----------------------------------------------------------------------------------------------------------------

FAMILIES = ("components", "thickness", "overhang", "blocking", "contacts", "reach", "tool", "geodesic")
LOCAL_CASES = {"local:K2": "random_r5_ofsolid", "local:K9": "random_r81_ofsolid", "local:K12": "random_r144_ofsolid",
               "local:2x3x64": "long_z64", "local:2x3x65": "long_z65"}       # k_thick_local<4>, <10>, <16>; the words' edge
TOOLS = {"2x3x64": tool.FLAT1, "2x3x65": tool.FLAT1, "3x5x130": tool.BALL3, "6x5x70": tool.STEEP}
CASES = collections.OrderedDict([
    ("components", ["noise", "line130", "2x3x64"]),
    ("thickness", ["z:3x5x130", "z:2x3x64", "z:2x3x65", "axis:y300", "axis:x300", "axis:x130", "axis:y5x130", "axis:y3x64"] + list(LOCAL_CASES)),
    ("overhang", ["noise", "5x7x64"]),
    ("blocking", ["5x7x130", "2x3x64"]),
    ("contacts", ["random", "one_line_65", "1x3x17", "2x3x64"]),
    ("reach", ["drain:9x8x130", "drain:9x8x64", "ground:two_ids", "ground:9x8x130", "ground:9x8x64"]),
    ("tool", list(TOOLS)),
    ("geodesic", ["5x7x130", "2x3x64", "1x1x70"]),
])
# the thickness passes: (K, cap) along z; (K, cap, tile) along x and y, tile + 2 K <= 256 so that both arms run
Z_PARAMS = ((8, 70), (65, 4226))
AXIS_PARAMS = {"y300": (96, 12000, 64), "x300": (10, 200, 236), "x130": (10, 200, 5), "y5x130": (3, 900, 4), "y3x64": (3, 900, 2)}
# the suite's axis volumes have nz = 21 and 16: for nz > 64 and nz % 64 == 0 the depth fields and the ids of the z lattices are
# walked along y, values around 1000 under a cap of 900, so that both sides of the cap are there to count
AXIS_FROM_Z = {"y5x130": "3x5x130", "y3x64": "2x3x64"}
CONTROL = {family: cases[0] for family, cases in CASES.items()}     # the case that also runs at the tight pitch


def _noise64(shape=(2, 3, 64)):
    """The 2x3x64 lattice of the tool cases at a density that leaves every family something to find."""
    return tool.noise(shape, 0.3)


@functools.lru_cache(maxsize=None)
def _cropped(kind, name, nz):
    """The first nz layers of z of a raw case of the reach or the overhang kernels: the suite has no lattice with nz % 64 == 0
    that is more than 2 x 3 across, where every sample is at a lateral border and in the first or the last layer."""
    ids = raw.over_ids(name) if kind == "over" else (drain if kind == "drain" else isl).raw_ids(name)
    ids = numpy.ascontiguousarray(ids[:, :, :nz])
    ids.setflags(write=False)
    return ids


def axis_of(name):
    return 1 if name in AXIS_FROM_Z else raw.AXIS_VOLUMES[name].axis


def axis_values(name):
    """The uint16 input of a pass along x or y."""
    return raw.z_depth(AXIS_FROM_Z[name]) if name in AXIS_FROM_Z else raw.axis_input(name)


@functools.lru_cache(maxsize=None)
def axis_ids(name):
    """Ids for the finishing passes over axis_values(name): raw.finish_ids() on x300, the z lattices' own, else the same recipe."""
    if name == "x300":
        return raw.finish_ids()
    if name in AXIS_FROM_Z:
        return raw.z_ids(AXIS_FROM_Z[name])
    shape = raw.AXIS_VOLUMES[name].shape
    rng = numpy.random.default_rng(6363 + sum(shape))
    ids = rng.integers(0, 64, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < 0.2] = 63
    ids[rng.random(shape) < 0.05] = EMPTY
    ids.setflags(write=False)
    return ids


def ids_of(family, case):
    """The raw ids of a case (the field of a thickness pass along x or y for "axis:" cases' shape)."""
    if family == "components":
        return raw.z_ids("2x3x64") if case == "2x3x64" else raw.comp_ids(case)
    if family == "thickness":
        kind, name = case.split(":")
        return raw.z_ids(name) if kind == "z" else axis_ids(name) if kind == "axis" else wall.RAW_BY_NAME[LOCAL_CASES[case]].ids
    if family == "overhang":
        return _cropped("over", "noise", 64) if case == "5x7x64" else raw.over_ids(case)
    if family == "blocking":
        return raw.block_small_ids() if case == "5x7x130" else _noise64()
    if family == "contacts":
        return _noise64() if case == "2x3x64" else con.raw_ids(case)
    if family == "reach":
        kind, name = case.split(":")
        scenes = drain if kind == "drain" else isl
        return _cropped(kind, "9x8x130", 64) if name == "9x8x64" else scenes.raw_ids(name)
    if family == "tool":
        return tool.noise((6, 5, 70), 0.3) if case == "6x5x70" else tool.noise(tuple(int(v) for v in case.split("x")), 0.3)
    if family == "geodesic":
        return geodesic_ids(case)
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def geodesic_ids(case):
    """flow_length_scenes.some_ids; every column ends with an empty sample, with part 3 or with another part in turn, so that
    under every `of` some column's top is in S and some is not."""
    shape = tuple(int(v) for v in case.split("x"))
    ids = flow.some_ids(numpy.random.default_rng(2700 + sum(shape)), shape)
    tops = numpy.array([3, EMPTY, 7], dtype=numpy.uint8)[numpy.arange(shape[0] * shape[1]) % 3].reshape(shape[:2])
    ids[:, :, -1] = tops if shape[0] * shape[1] > 1 else 3
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def geodesic_field(case, of):
    """flow_length_scenes.some_field, no distance field, for the sweeps and the statistics; NONE on every top that is in S, which
    the zeros of the padding would lower."""
    ids = geodesic_ids(case)
    s = flow.in_set_of(ids, of)
    field = flow.some_field(numpy.random.default_rng(2800 + sum(ids.shape)), ids.shape, s)
    field[:, :, -1] = numpy.where(s[:, :, -1], NONE, field[:, :, -1])
    field.setflags(write=False)
    return field


def geodesic_poison(of):
    """Ids that are in S: read as data they would carry a way through the padding and be counted."""
    return raw.alternating(0, 63) if of == SOLID else raw.constant(EMPTY if of == flow.EMPTY_SPACE else of)


def geodesic_samples(case, of):
    """The listed seeds: the first and the last samples of S, two outside it, a corner twice."""
    ids = geodesic_ids(case)
    s = flow.in_set_of(ids, of)
    inside, outside = numpy.argwhere(s), numpy.argwhere(~s)
    corner = tuple(n - 1 for n in ids.shape)
    return [tuple(int(v) for v in p) for p in list(inside[:1]) + list(outside[:2]) + list(inside[-2:])] + [corner, corner]


def ground_of(case):
    return isl.RAW_OF.get(case.split(":")[1], SOLID)


def arms(family, case):
    if family == "components":
        return [(local, solid) for local in (0, 1) for solid in (0, 1)]
    if family == "thickness":
        kind, name = case.split(":")
        if kind == "z":
            # (2x3x64 has no sample of a single part at the top of a column: nothing there for that part's poison to change)
            return [(1, of) + p for of in ((SOLID,) if name == "2x3x64" else (SOLID, 63)) for p in Z_PARAMS] + [(2, SOLID) + p for p in Z_PARAMS]
        if kind == "axis":                                                        # (finish, of, outside)
            return [(0, SOLID, "zero"), (0, SOLID, "half"), (1, SOLID, "cap"), (2, SOLID, "cap"), (2, 63, "cap")]
        return [()]
    if family == "overhang":
        # (the whole reach over part 63 bites where "noise" plants its overhangs in the layer z = nz - 1)
        return [(axis, up, reach_sq, of) for axis, up in dis.DIRECTIONS
                for reach_sq, of in ((1, SOLID), (1, 63)) + (((8, 63),) if case == "noise" else ())]
    if family == "blocking":
        return [(64,), (40,)]
    if family == "contacts":
        return [()]
    if family == "reach":
        return list(dis.DIRECTIONS)
    if family == "tool":
        # (along x and y the padding adds columns: under SOLID they change nothing the lattice's columns see in some cases)
        return [(axis, up, 63) for axis, up in dis.DIRECTIONS] + [(2, True, SOLID), (2, False, SOLID)]
    if family == "geodesic":
        # (the one line holds one part at its top: in S for SOLID and for 3)
        return [(of,) for of in ((SOLID, 3) if case == "1x1x70" else (SOLID, 3, flow.EMPTY_SPACE))]
    raise KeyError(family)


def blind(family, case, arm):
    return family == "thickness" and case.startswith("axis:") and arm[0] == 0


def inputs(family, case, arm, pitch=None):
    """The poisoned device images of a case's inputs at `pitch` (ceil16(nz) without one): ordered dict name -> array."""
    ids = ids_of(family, case)
    out = collections.OrderedDict()
    if family == "components":
        out["ids"] = raw.padded(ids, raw.COMP_POISON, pitch)[0]
    elif family == "thickness":
        kind, name = case.split(":")
        if kind == "z":
            if arm[0] == 1:
                out["ids"] = raw.padded(ids, raw.z_ids_poison(arm[1]), pitch)[0]
            else:
                out["depth"] = raw.padded16(raw.z_depth(name), raw.Z_DEPTH_POISON, pitch)[0]
        elif kind == "axis":
            of = arm[1]
            out["in"] = raw.padded16(axis_values(name), raw.constant(0) if arm[0] == 0 else raw.AXIS_COUNTED_POISON, pitch)[0]
            out["ids"] = raw.padded(ids, raw.constant(raw.code(of) if of != SOLID else 0), pitch)[0]    # in S: it would be counted
        else:
            out["ids"], out["depth"], _ = wall.raw_buffers(wall.RAW_BY_NAME[LOCAL_CASES[case]], pitch)
    elif family == "overhang":
        out["ids"] = raw.padded(ids, raw.OVER_POISON, pitch)[0]
    elif family == "blocking":
        out["ids"] = raw.padded(ids, raw.BLOCK_POISON, pitch)[0]
    elif family == "contacts":
        out["ids"] = raw.padded(ids, raw.CONTACT_POISON, pitch)[0]
    elif family == "reach":
        out["ids"] = raw.padded(ids, raw.DRAIN_POISON if case.startswith("drain:") else raw.ground_poison(ground_of(case)), pitch)[0]
    elif family == "tool":
        out["ids"] = raw.padded(ids, tool.RAW_POISON, pitch)[0]
    elif family == "geodesic":
        out["ids"] = raw.padded(ids, geodesic_poison(arm[0]), pitch)[0]
        out["dist"] = flow.padded32(geodesic_field(case, arm[0]), raw.constant(0), pitch)[0]      # 0 in the padding: it would seed
    return out


@functools.lru_cache(maxsize=None)
def _layers(case, axis):
    """The layers' labels of a reach case: the same up and down."""
    ids = ids_of("reach", case)
    if case.startswith("drain:"):
        return drain.layer_labels(ids == EMPTY, axis)
    return isl.layer_labels(thin.in_set_of(ids, ground_of(case)), axis)


def _counts(mask, ids):
    return [int((mask & (ids == p)).sum()) for p in range(64)]


def _reference(family, case, arm, given, labels=True):
    """The reference over `given`, the inputs as arrays whose every entry is data; `labels`: the layers' labels too."""
    ref = collections.OrderedDict()
    ids = given.get("ids")
    if family == "components":
        local, solid = arm
        r = comp.reference_components(ids, SOLID if solid else comp.EMPTY_SPACE)
        ref["labels"] = ("labels", r.labels)
        ref["components"] = ("table", [tuple(c) for c in r.components])
    elif family == "thickness":
        kind, name = case.split(":")
        if kind == "z":
            transform, of, K, cap = arm
            if transform == 1:
                ref["out"] = ("volume", thin.min_plus_1d(raw.z_input_1(ids, of, cap), 2, K, cap, 0))
            else:
                ref["out"] = ("volume", thin.min_plus_1d(raw.z_input_2(given["depth"], cap), 2, K, cap, cap))
        elif kind == "axis":
            finish, of, which = arm
            K, cap, tile = AXIS_PARAMS[name]
            out = thin.min_plus_1d(given["in"], axis_of(name), K, cap, raw.outside_of(which, cap))
            reached = out == cap
            if finish != 2:
                ref["out"] = ("volume", out)
            if finish == 1:
                ref["counts"] = ("table", _counts(reached, ids))                  # (ids up to 63; an empty sample is nobody's)
            if finish == 2:
                marked = reached & thin.in_set_of(ids, of)
                ref["thin"] = ("volume", numpy.where(marked, ids, EMPTY).astype(numpy.uint8))
                ref["counts"] = ("table", _counts(marked, ids))
        else:
            c = wall.RAW_BY_NAME[LOCAL_CASES[case]]
            s = thin.in_set_of(ids, c.of)
            out = wall.raw_local(given["depth"], s, c.r2)
            ref["out"] = ("volume", out)
            ref["keys"] = ("table", [int(k) for k in wall.keys_of(numpy.where(s, ids, EMPTY), out)])
            ref["counts"] = ("table", _counts((out == c.r2 + 1) & s, ids))
    elif family == "overhang":
        axis, up, reach_sq, of = arm
        r = over.reference_overhangs(ids, axis, up, reach_sq, of, 64)
        ref["overhang"], ref["support"], ref["landing"] = ("volume", r.overhang_ids), ("volume", r.support_ids), ("volume", r.landing_ids)
        ref["word"] = ("table", [ids.shape[axis] - r.first_layer])
        ref["overhang_counts"], ref["support_counts"] = ("table", list(r.overhang_counts)), ("table", list(r.support_counts))
        ref["landing_counts"], ref["plate"] = ("table", list(r.landing_counts)), ("table", [r.plate_landings])
    elif family == "blocking":
        n, = arm
        distance, witness = dis.reference_blocking(numpy.where(ids < n, ids, EMPTY).astype(numpy.uint8), n)
        ref["distance"], ref["witness"] = ("table", distance), ("table", witness)
    elif family == "contacts":
        faces, sums, box, witness, exposed, contact_ids, contact_counts = con.reference_faces(ids, con.RAW_PARTS)
        for name, value in (("faces", faces), ("sums", sums), ("box", box), ("witness", witness), ("exposed", exposed)):
            ref[name] = ("table", value)
        ref["contact_ids"], ref["contact_counts"] = ("volume", contact_ids), ("table", list(contact_counts))
    elif family == "reach":
        axis, up = arm
        if case.startswith("drain:"):
            empty = ids == EMPTY                                                  # drainage_scenes.reference_of without the pools
            escapes = drain.escape_set(empty, axis, up)
            trapped_ids = numpy.where(empty & ~escapes, drain.floors(ids, axis, up), EMPTY).astype(numpy.uint8)
            ref["layers"] = ("labels", _layers(case, axis) if labels else None)
            ref["flagged"], ref["trapped"] = ("volume", escapes), ("volume", trapped_ids)
            ref["counts"] = ("table", [int((trapped_ids == p).sum()) for p in range(64)])
        else:
            of = ground_of(case)
            s, sign = thin.in_set_of(ids, of), 1 if up else -1                    # islands_scenes.reference_of without the islands
            g = isl.grounded_set(s, axis, up)
            f = s & ~g
            sets = {"floating": f, "start": f & ~isl.shifted(s, axis, sign), "join": f & isl.shifted(g, axis, -sign)}
            ref["layers"] = ("labels", _layers(case, axis) if labels else None)
            ref["word"] = ("table", [ids.shape[axis] - isl.first_layer(s, axis, up)])
            ref["flagged"] = ("volume", g)
            for name, m in sets.items():
                ref[name] = ("volume", numpy.where(m, ids, EMPTY).astype(numpy.uint8))
                ref[name + "_counts"] = ("table", _counts(m, ids))
    elif family == "tool":
        axis, up, of = arm
        r = tool.reference_tool_access(ids, axis, up, TOOLS[case], of, 64, pockets=False)
        along = "table" if axis == 2 else "field"
        ref["keys"] = (along, numpy.where(r.tops > 0, r.tops * 256 + (255 - r.top_ids.astype(numpy.int64)), 0))
        ref["tips"] = ("table" if axis == 2 else "tips", r.tips)
        ref["cut"], ref["crowd"] = (along, r.cut), (along, r.crowd)
        ref["rest"] = ("volume", r.rest_ids)
        ref["undercut_counts"], ref["tight_counts"] = ("table", list(r.undercut_counts)), ("table", list(r.tight_counts))
    elif family == "geodesic":
        of, = arm
        s = flow.in_set_of(ids, of)
        shape = ids.shape
        last = tuple(n - 1 for n in ids_of(family, case).shape)                    # the layers and the samples are the LATTICE's
        ref["seed_border"] = ("volume", flow.seeded(s, flow.border_of(shape)))
        for axis in range(3):
            ref["seed_layer%d" % axis] = ("volume", flow.seeded(s, flow.layer_of(shape, axis, last[axis])))
        ref["seed_list"] = ("volume", flow.seeded(s, flow.listed(shape, geodesic_samples(case, of))))
        lowered = []
        for axis in range(3):
            out, low = flow.swept(given["dist"], s, axis)
            ref["swept%d" % axis] = ("volume", out)
            lowered.append(int(low))
        ref["lowered"] = ("table", lowered)
        keys, counts = flow.raw_stats(ids, of, given["dist"], shape[2])
        ref["counts"] = ("table", counts.tolist())
        far = []
        for key in keys.tolist():
            q = 0xffffffff - (key & 0xffffffff)
            far.append((key >> 32,) + tuple(int(v) for v in numpy.unravel_index(q, shape)) if key else (0, 0, 0, 0))
        ref["far"] = ("far", far)
    return ref


def reference(family, case, arm, widen=None):
    """See the module's docstring.  Computed once and shared; nobody changes it."""
    if family == "components":
        arm = (0, arm[1])                                                         # (the reference knows no `local`)
    return _shared_reference(family, case, arm, widen)


@functools.lru_cache(maxsize=None)
def _shared_reference(family, case, arm, widen):
    if widen is None:
        given = collections.OrderedDict((name, a[:, :, :ids_of(family, case).shape[2]]) for name, a in inputs(family, case, arm).items())
    else:
        given = inputs(family, case, arm, widen)
    return _reference(family, case, arm, given, widen is None)


def widened_differs(family, case, arm, pitch):
    """Does the reference over the padding as data differ from the true one on the lattice, or in a count or a table?"""
    nz = ids_of(family, case).shape[2]
    true, wide = reference(family, case, arm), reference(family, case, arm, pitch)
    assert list(true) == list(wide)
    for name, (kind, want) in true.items():
        other = wide[name][1]
        if kind in ("volume", "field"):
            other = other[..., :nz]
        elif kind in ("labels", "tips", "far"):
            continue
        if mismatches(other, want, 1):
            return True
    return False


def tool_dims(case, axis):
    """(nu, nv, K) of a tool case along `axis`."""
    shape = ids_of("tool", case).shape
    nu, nv = (shape[a] for a in range(3) if a != axis)
    return nu, nv, math.isqrt(TOOLS[case].radius_sq)


def combinations():
    """Every (family, case, placement name) the device test runs: word and segment for all, tight for a family's control."""
    out = []
    for family, cases in CASES.items():
        out += [(family, case, p) for case in cases for p in ("word", "segment")]
        out.append((family, CONTROL[family], "tight"))
    return out
