"""The id-volume entry points of include/hip_util.h at every pitch and alignment their contract allows: the 27 entry points of
instance_components.hip, instance_thickness.hip, instance_local.hip, instance_overhang.hip, instance_blocking.hip,
instance_contacts.hip, instance_reach.hip, instance_tool.hip and instance_geodesic.hip over the buffers of pitched_buffers.py
-- a pitch one word and more than one 64-sample segment beyond ceil16(nz), every pointer aligned to what its entry point asks for and to no more, the
whole padding poisoned, sentinels in every output's padding and in guard zones around every buffer -- against the NumPy
references of the raw cases, which know nothing of a pitch.  Every output is EQUAL to its reference, entry for entry; every byte
of an output's padding still holds the sentinel (the labels' padding: NONE, which hu_components_local, hu_drain_layers and
hu_ground_layers write there, as include/hip_util.h says); both guards of every buffer, inputs included, are untouched; and no
accumulator beyond the parts in use has moved.  One case per family also runs at the tight pitch, the control: a failure there
is the placement machinery's.  (test_pitch_alignment_host.py shows on the CPU that the cases hold their edges.)

hu_assembly_voxels_cells and hu_assembly_voxels_leaf need a cell traversal, not a raw volume: the fill itself is still only run
at the tight pitch of assembly_voxels.volume_shape."""
import ctypes
import math
import sys

import numpy
import pytest

from codecad_amd.hip_util import check

import pitched_buffers as pb
import raw_volume_scenes as raw
from pitched_buffers import Placed, SENTINEL, SOLID, EMPTY, NONE

pytestmark = pytest.mark.gpu
components = sys.modules["codecad_amd.assembly_components"]
disassembly = sys.modules["codecad_amd.disassembly"]
contacts = sys.modules["codecad_amd.contacts"]
FLAG = 0x80000000
ONES64 = 0xffffffffffffffff


LIVE = []                       # the runs of the arm under way: the test releases them whatever happens


class Run:
    """The buffers of one arm: placed, named, read back once, checked together."""

    def __init__(self, hip, placement, shape):
        LIVE.append(self)
        self.hip, self.placement, self.shape = hip, placement, shape
        self.nz = shape[2]
        self.pitch = placement.pitch_of(self.nz)
        self.dims = (ctypes.c_uint32 * 3)(*shape)
        self.placed = {}                                                           # name -> (Placed, what its padding must hold)
        self.got = {}

    def volume(self, name, host, align):
        """An input volume, poisoned by pitched_buffers.inputs."""
        assert host.shape[2] == self.pitch
        self.placed[name] = (Placed(self.hip.queue, host, align, self.placement, self.nz), None)
        return self.placed[name][0].ptr

    def out_volume(self, name, dtype, align, padding=None):
        """An output volume of sentinels; `padding`: what the padding holds afterwards where that is not the sentinel."""
        host = pb.sentinel(dtype, self.shape[:2] + (self.pitch,))
        want = pb.sentinel(dtype, (1,))[0] if padding is None else padding
        self.placed[name] = (Placed(self.hip.queue, host, align, self.placement, self.nz), want)
        return self.placed[name][0].ptr

    def array(self, name, host, align):
        """Anything that is no volume: accumulators, words, tables, fields."""
        self.placed[name] = (Placed(self.hip.queue, host, align, self.placement), None)
        return self.placed[name][0].ptr

    def read(self):
        """name -> the lattice's part of every buffer, after the paddings and the guards were checked."""
        out = {}
        for name, (p, padding) in self.placed.items():
            lattice, rest, guards = p.read()
            assert (guards[0] == SENTINEL).all() and (guards[1] == SENTINEL).all(), (name, "a guard zone was written")
            if padding is not None:
                wrong = numpy.argwhere(rest != padding)
                assert len(wrong) == 0, (name, "padding", [(tuple(int(v) for v in k), int(rest[tuple(k)])) for k in wrong[:8]])
            out[name] = lattice
        return out

    def release(self):
        for p, _ in self.placed.values():
            p.release()


def compare(got, ref, where):
    assert list(got) == [name for name in ref], (where, list(got), list(ref))
    for name, (kind, want) in ref.items():
        wrong = pb.mismatches(got[name], want)
        assert not wrong, (where, name, wrong)


def zeros(n):
    return numpy.zeros(n, dtype=numpy.uint64)


# ---- the families: each runs one arm of one case and returns what the reference names -------------------------------------

def run_components(hip, case, arm, placement):
    local, solid = arm
    ids = pb.ids_of("components", case)
    r = Run(hip, placement, ids.shape)
    lib, s, pitch, dims = hip.lib, hip.queue.handle, r.pitch, r.dims
    volume = r.volume("ids", pb.inputs("components", case, arm, pitch)["ids"], 16)
    labels = r.out_volume("labels", numpy.uint32, 4, padding=NONE)
    check(lib.hu_components_local(volume, labels, dims, pitch, solid, local, s), "hu_components_local")
    check(lib.hu_components_merge(labels, dims, pitch, local, s), "hu_components_merge")
    check(lib.hu_components_flatten(labels, dims, pitch, s), "hu_components_flatten")
    want = pb.reference("components", case, arm)
    capacity = len(want["components"][1])
    counter = r.array("counter", numpy.zeros(1, dtype=numpy.uint32), 4)
    table = r.array("table", numpy.zeros(capacity + 2, dtype=components._ROW), 8)    # two rows beyond the components: not touched
    check(lib.hu_components_stats(volume, labels, dims, pitch, solid, 1, counter, table, capacity + 2, s), "hu_components_stats")
    check(lib.hu_components_finish(labels, dims, pitch, s), "hu_components_finish")
    back = r.read()
    assert int(back["counter"][0]) == capacity, (int(back["counter"][0]), capacity)
    rows = back["table"]
    assert rows[capacity:].tobytes() == bytes(2 * components._ROW.itemsize)         # nothing beyond the rows in use has moved
    found = components._components(rows[:capacity], (0.0, 0.0, 0.0), 1.0)
    return {"labels": back["labels"], "components": [(c.label, c.count, c.box, c.index_sums, c.touches_border, c.parts) for c in found]}


def run_thickness(hip, case, arm, placement):
    kind, name = case.split(":")
    ids = pb.ids_of("thickness", case)
    lib, s = hip.lib, hip.queue.handle
    given = None
    arms = []
    if kind == "z":
        transform, of, K, cap = arm
        for lds in (0, 1):
            r = Run(hip, placement, ids.shape)
            given = pb.inputs("thickness", case, arm, r.pitch)
            volume = r.volume("ids", given["ids"], 1) if transform == 1 else None
            depth = r.volume("depth", given["depth"], 2) if transform == 2 else None
            out = r.out_volume("out", numpy.uint16, 2)
            check(lib.hu_thickness_pass_z(volume, depth, out, r.dims, r.pitch, raw.code(of), raw.RADIUS_SQ, K, cap, lds, s), "hu_thickness_pass_z")
            back = r.read()
            arms.append({"out": back["out"]})
    elif kind == "axis":
        finish, of, which = arm
        K, cap, tile = pb.AXIS_PARAMS[name]
        axis = pb.axis_of(name)
        for lds in (0, 1):
            r = Run(hip, placement, ids.shape)
            given = pb.inputs("thickness", case, arm, r.pitch)
            source, volume = r.volume("in", given["in"], 2), r.volume("ids", given["ids"], 1)
            out, marked = r.out_volume("out", numpy.uint16, 2), r.out_volume("thin", numpy.uint8, 1)
            counts = r.array("counts", zeros(64), 8)
            check(lib.hu_thickness_pass_axis(source, out if finish != 2 else None, volume if finish else None, marked if finish == 2 else None,
                                             counts if finish else None, r.dims, r.pitch, axis, raw.code(of), K, cap, raw.outside_of(which, cap),
                                             finish, tile, lds, s), "hu_thickness_pass_axis")
            back = r.read()
            got = {}
            if finish != 2:
                got["out"] = back["out"]
                assert (back["thin"] == SENTINEL).all()
            else:
                assert (back["out"] == 0xa5a5).all()                                # finish = 2 leaves out_dev alone
            if finish == 1:
                got["counts"] = [int(v) for v in back["counts"]]
            if finish == 2:
                got["thin"], got["counts"] = back["thin"], [int(v) for v in back["counts"]]
            if finish == 0:
                assert not back["counts"].any()
            arms.append(got)
    else:
        c = pb.wall.RAW_BY_NAME[pb.LOCAL_CASES[case]]
        for lds in (1, 0):
            r = Run(hip, placement, ids.shape)
            given = pb.inputs("thickness", case, arm, r.pitch)
            depth, volume = r.volume("depth", given["depth"], 2), r.volume("ids", given["ids"], 1)
            out = r.out_volume("out", numpy.uint16, 2)
            keys, counts = r.array("keys", numpy.full(64, ONES64, dtype=numpy.uint64), 8), r.array("counts", zeros(64), 8)
            check(lib.hu_thickness_local(depth, volume, out, keys, counts, r.dims, r.pitch, raw.code(c.of), c.r2, lds, s), "hu_thickness_local")
            back = r.read()
            arms.append({"out": back["out"], "keys": [int(v) for v in back["keys"]], "counts": [int(v) for v in back["counts"]]})
    for name in arms[0]:                                                            # the two arms give the same bytes
        assert numpy.asarray(arms[0][name]).tobytes() == numpy.asarray(arms[1][name]).tobytes(), name
    return arms[0]


def run_overhang(hip, case, arm, placement):
    axis, up, reach_sq, of = arm
    ids = pb.ids_of("overhang", case)
    r = Run(hip, placement, ids.shape)
    lib, s, pitch, dims = hip.lib, hip.queue.handle, r.pitch, r.dims
    volume = r.volume("ids", pb.inputs("overhang", case, arm, pitch)["ids"], 1)
    marks, support, landing = (r.out_volume(name, numpy.uint8, 1) for name in ("overhang", "support", "landing"))
    word = r.array("word", numpy.zeros(1, dtype=numpy.uint32), 4)
    mark_counts, column_counts = r.array("mark_counts", zeros(64), 8), r.array("column_counts", zeros(129), 8)
    code = raw.code(of)
    check(lib.hu_overhang_first_layer(volume, word, dims, pitch, axis, int(up), code, s), "hu_overhang_first_layer")
    check(lib.hu_overhang_mark(volume, marks, word, mark_counts, dims, pitch, axis, int(up), reach_sq, code, s), "hu_overhang_mark")
    check(lib.hu_overhang_columns(volume, marks, support, landing, word, column_counts, dims, pitch, axis, int(up), code, s), "hu_overhang_columns")
    back = r.read()
    columns = [int(v) for v in back["column_counts"]]
    return {"overhang": back["overhang"], "support": back["support"], "landing": back["landing"], "word": [int(back["word"][0])],
            "overhang_counts": [int(v) for v in back["mark_counts"]], "support_counts": columns[:64], "landing_counts": columns[64:128],
            "plate": columns[128:]}


def run_blocking(hip, case, arm, placement):
    n, = arm
    ids = pb.ids_of("blocking", case)
    r = Run(hip, placement, ids.shape)
    volume = r.volume("ids", pb.inputs("blocking", case, arm, r.pitch)["ids"], 1)
    keys = r.array("keys", numpy.full(disassembly._KEYS, ONES64, dtype=numpy.uint64), 8)
    for axis in range(3):
        check(hip.lib.hu_blocking_lines(volume, keys, r.dims, r.pitch, axis, n, hip.queue.handle), "hu_blocking_lines")
    table = r.read()["keys"]
    assert (table[:, n:] == ONES64).all() and (table[:, :, n:] == ONES64).all()     # nothing beyond the n parts is touched
    distance, witness = disassembly._decode(table, n)
    return {"distance": distance, "witness": witness}


def run_contacts(hip, case, arm, placement):
    ids = pb.ids_of("contacts", case)
    n = pb.con.RAW_PARTS
    arms = []
    for with_volume in (True, False):
        r = Run(hip, placement, ids.shape)
        volume = r.volume("ids", pb.inputs("contacts", case, arm, r.pitch)["ids"], 1)
        out = r.out_volume("contact_ids", numpy.uint8, 1)
        rows = r.array("rows", numpy.zeros(contacts._ROWS, dtype=contacts._ROW), 8)
        counts = r.array("counts", zeros(7 * 64).reshape(contacts._COUNTS), 8)
        check(hip.lib.hu_contact_faces(volume, out if with_volume else None, rows, counts, r.dims, r.pitch, n, hip.queue.handle), "hu_contact_faces")
        back = r.read()
        faces, sums, box, witness = contacts._decode(back["rows"], n)
        totals = back["counts"]
        arms.append({"faces": faces, "sums": sums, "box": box, "witness": witness, "exposed": numpy.ascontiguousarray(totals[:6, :n].reshape(3, 2, n)),
                     "contact_ids": back["contact_ids"], "contact_counts": [int(v) for v in totals[6, :n]]})
    assert (arms[1].pop("contact_ids") == SENTINEL).all()                            # with NULL nothing is written
    for name, value in arms[1].items():                                             # ... and the tables are the same
        assert not pb.mismatches(value, arms[0][name]), name
    return arms[0]


def flagged_of(entries, members):
    """bool like `members`: the members whose root's entry has bit 31 set, from a label buffer read back after a flatten."""
    flat = entries.ravel()
    own = entries[:, :, :members.shape[2]]
    root = numpy.where(members, own & (FLAG - 1), 0)                                 # a root's own entry may carry the flag
    return members & (((own & FLAG) != 0) | ((flat[root] & FLAG) != 0))


def run_reach(hip, case, arm, placement):
    axis, up = arm
    ground = case.startswith("ground:")
    ids = pb.ids_of("reach", case)
    of = pb.ground_of(case) if ground else None
    members = pb.thin.in_set_of(ids, of) if ground else ids == EMPTY
    r = Run(hip, placement, ids.shape)
    lib, s, pitch, dims, nz = hip.lib, hip.queue.handle, r.pitch, r.dims, r.nz
    image = pb.inputs("reach", case, arm, pitch)["ids"]
    volume = r.volume("ids", image, 16)
    bytewise = r.volume("ids at any address", image, 1)                              # hu_drain_floor asks for no alignment of its ids
    labels = r.out_volume("labels", numpy.uint32, 4, padding=NONE)
    changed = r.array("changed", numpy.zeros(1, dtype=numpy.uint32), 4)
    code = raw.code(of) if ground else None
    if ground:
        depth = r.array("word", numpy.zeros(1, dtype=numpy.uint32), 4)
        check(lib.hu_overhang_first_layer(volume, depth, dims, pitch, axis, int(up), code, s), "hu_overhang_first_layer")
    layers = []
    for local in (0, 1):                                                            # stage 1, both arms: the same labels
        r.placed["labels"][0].refill(pb.sentinel(numpy.uint32, ids.shape[:2] + (pitch,)))
        if ground:
            check(lib.hu_ground_layers(volume, labels, dims, pitch, axis, code, local, s), "hu_ground_layers")
        else:
            check(lib.hu_drain_layers(volume, labels, dims, pitch, axis, local, s), "hu_drain_layers")
        check(lib.hu_components_flatten(labels, dims, pitch, s), "hu_components_flatten")
        lattice, padding, _ = r.placed["labels"][0].read()
        assert (padding == NONE).all() and (lattice[~members] == NONE).all(), local
        layers.append(numpy.where(members, pb.linear_index(lattice, nz, pitch), NONE).astype(numpy.uint32))   # from the PLACED pitch
    assert numpy.array_equal(layers[0], layers[1])
    if ground:
        check(lib.hu_ground_seed(labels, depth, dims, pitch, axis, int(up), s), "hu_ground_seed")
    else:
        check(lib.hu_drain_seed(labels, dims, pitch, axis, int(up), s), "hu_drain_seed")
    for passes in range(1, ids.shape[axis] + 3):                                    # the rise, to its fixed point
        r.placed["changed"][0].refill(numpy.zeros(1, dtype=numpy.uint32))
        check(lib.hu_drain_rise(labels, changed, dims, pitch, axis, int(up), s), "hu_drain_rise")
        if not int(r.placed["changed"][0].read()[0][0]):
            break
    assert passes <= ids.shape[axis] + 1
    lattice, padding, _ = r.placed["labels"][0].read()
    entries = numpy.concatenate([lattice, padding], axis=2)
    got = {"layers": layers[0]}
    if ground:
        outs = [r.out_volume(name, numpy.uint8, 1) for name in ("floating", "start", "join")]
        counts = r.array("counts", zeros(3 * 64), 8)
        check(lib.hu_ground_mark(volume, labels, outs[0], outs[1], outs[2], counts, dims, pitch, axis, int(up), code, s), "hu_ground_mark")
    else:
        trapped, counts = r.out_volume("trapped", numpy.uint8, 1), r.array("counts", zeros(64), 8)
        check(lib.hu_drain_floor(bytewise, labels, trapped, counts, dims, pitch, axis, int(up), s), "hu_drain_floor")
    back = r.read()
    assert int(back["changed"][0]) == 0
    totals = [int(v) for v in back["counts"]]
    if ground:
        got["word"] = [int(back["word"][0])]
        got["flagged"] = flagged_of(entries, members)
        for k, name in enumerate(("floating", "start", "join")):
            got[name], got[name + "_counts"] = back[name], totals[64 * k:64 * k + 64]
    else:
        got["flagged"], got["trapped"], got["counts"] = flagged_of(entries, members), back["trapped"], totals
    return got


def run_tool(hip, case, arm, placement):
    axis, up, of = arm
    ids = pb.ids_of("tool", case)
    cutter = pb.TOOLS[case]
    nu, nv, K = pb.tool_dims(case, axis)
    r = Run(hip, placement, ids.shape)
    lib, s, pitch, dims = hip.lib, hip.queue.handle, r.pitch, r.dims
    volume = r.volume("ids", pb.inputs("tool", case, arm, pitch)["ids"], 16)
    rest = r.out_volume("rest", numpy.uint8, 16)
    tops, cut = (r.array(name, pb.sentinel(numpy.uint32, (nu, nv)), 4) for name in ("tops", "cut"))
    tips = r.array("tips", pb.sentinel(numpy.uint32, (nu + 2 * K, nv + 2 * K)), 4)
    profile = r.array("profile", numpy.array(cutter.profile, dtype=numpy.uint16), 2)
    counts = r.array("counts", zeros(128), 8)
    code = raw.code(of)
    check(lib.hu_tool_tops(volume, tops, dims, pitch, axis, int(up), code, s), "hu_tool_tops")
    check(lib.hu_tool_dilate(tops, profile, tips, nu, nv, cutter.radius_sq, s), "hu_tool_dilate")
    check(lib.hu_tool_erode(tips, tops, profile, cut, nu, nv, cutter.radius_sq, s), "hu_tool_erode")
    check(lib.hu_tool_rest(volume, tops, cut, rest, counts, dims, pitch, axis, int(up), code, s), "hu_tool_rest")
    back = r.read()
    assert numpy.array_equal(back["profile"], numpy.array(cutter.profile, dtype=numpy.uint16))
    totals = [int(v) for v in back["counts"]]
    return {"keys": back["tops"], "tips": back["tips"], "cut": back["cut"] >> 8, "crowd": back["cut"] & 255, "rest": back["rest"],
            "undercut_counts": totals[:64], "tight_counts": totals[64:]}


def run_geodesic(hip, case, arm, placement):
    """hu_geodesic_seed in its three modes, hu_geodesic_sweep on each axis and hu_geodesic_stats: the distances, the changed word
    and the samples aligned to 4 bytes and no more, the keys and the counts to 8, the ids at an odd address (they have no check);
    the padding of the distances holds 0, which would seed, and still holds it afterwards."""
    of, = arm
    ids = pb.ids_of("geodesic", case)
    flow = pb.flow
    r = Run(hip, placement, ids.shape)
    lib, s, pitch, dims = hip.lib, hip.queue.handle, r.pitch, r.dims
    given = pb.inputs("geodesic", case, arm, pitch)
    volume = r.volume("ids", given["ids"], 1)
    host = pb.sentinel(numpy.uint32, ids.shape[:2] + (pitch,))                       # every in-lattice entry is written by a seed
    host[:, :, r.nz:] = 0
    r.placed["dist"] = (Placed(hip.queue, host, 4, placement, r.nz), 0)
    dist = r.placed["dist"][0].ptr
    rows = numpy.array(pb.geodesic_samples(case, of), dtype=numpy.uint32)
    samples = r.array("samples", rows, 4)
    word = r.array("word", numpy.zeros(1, dtype=numpy.uint32), 4)
    keys, counts = r.array("keys", zeros(65), 8), r.array("counts", zeros(3 * 65).reshape(3, 65), 8)
    code = flow.code(of)
    got = {}

    def field():
        lattice, padding, _ = r.placed["dist"][0].read()
        assert (padding == 0).all()
        return lattice

    last = [n - 1 for n in ids.shape]
    check(lib.hu_geodesic_seed(volume, dist, dims, pitch, code, flow.MODE_BORDER, 0, 0, None, 0, s), "hu_geodesic_seed")
    got["seed_border"] = field()
    for axis in range(3):
        check(lib.hu_geodesic_seed(volume, dist, dims, pitch, code, flow.MODE_LAYER, axis, last[axis], None, 0, s), "hu_geodesic_seed")
        got["seed_layer%d" % axis] = field()
    check(lib.hu_geodesic_seed(volume, dist, dims, pitch, code, flow.MODE_LIST, 0, 0, samples, len(rows), s), "hu_geodesic_seed")
    got["seed_list"] = field()
    lowered = []
    for axis in range(3):
        r.placed["dist"][0].refill(given["dist"])
        r.placed["word"][0].refill(numpy.zeros(1, dtype=numpy.uint32))
        check(lib.hu_geodesic_sweep(volume, dist, word, dims, pitch, axis, code, s), "hu_geodesic_sweep")
        got["swept%d" % axis] = field()
        lowered.append(int(r.placed["word"][0].read()[0][0] != 0))
    got["lowered"] = lowered
    r.placed["dist"][0].refill(given["dist"])
    check(lib.hu_geodesic_stats(volume, dist, keys, counts, dims, pitch, code, s), "hu_geodesic_stats")
    back = r.read()
    assert numpy.array_equal(back["dist"], given["dist"][:, :, :r.nz]) and numpy.array_equal(back["samples"], rows)   # the statistics write no distance
    got["counts"] = back["counts"].tolist()
    far = []
    for key in back["keys"].tolist():                                               # the key's buffer index, by the PLACED pitch
        q = 0xffffffff - (key & 0xffffffff)
        far.append((key >> 32, q // pitch // ids.shape[1], q // pitch % ids.shape[1], q % pitch) if key else (0, 0, 0, 0))
    got["far"] = far
    return got


RUNNERS = {"components": run_components, "thickness": run_thickness, "overhang": run_overhang, "blocking": run_blocking,
           "contacts": run_contacts, "reach": run_reach, "tool": run_tool, "geodesic": run_geodesic}


@pytest.mark.parametrize("family,case,placement", pb.combinations(), ids=lambda v: str(v).replace(":", "_"))
def test_every_output_equals_the_reference_wherever_the_buffers_lie(hip, family, case, placement):
    place = pb.PLACEMENTS[placement]
    nz = pb.ids_of(family, case).shape[2]
    print(family, case, placement, "nz", nz, "pitch", place.pitch_of(nz), "arms", len(pb.arms(family, case)))
    for arm in pb.arms(family, case):
        try:
            got = RUNNERS[family](hip, case, arm, place)
        finally:                                                                    # (a failed check leaves no allocation behind)
            while LIVE:
                LIVE.pop().release()
        compare(got, pb.reference(family, case, arm), (family, case, placement, arm))
