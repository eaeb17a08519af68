"""The references and the scenarios of test_gpu_drainage.py, and the host side of drainage(), checked without a device.

drainage_scenes.escape_set is written from the definition: seeds, then growth by shifted arrays to the fixed point.  That the
layer-by-layer restatement gives the same set on every scene, direction and raw volume, that the consequences the module's
docstring lists hold, and that both give the values written by hand, come first.  Then the synchronous steps, the flip, the
driver over a recording library, the C ABI, the entry points' refusals and the kernels' resources."""
import ctypes
import os
import re
import sys
import types

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes
from codecad_amd.hip_util import _lib

import assembly_components_scenes as comp
import disassembly_scenes as dis_scenes
import drainage_scenes as scenes
import reach_kernels as reach
from drainage_scenes import SCENES, MINE, CASES, RAW_CASES, DIRECTIONS, reference, raw_reference, scene, EMPTY, NONE

dr = sys.modules["codecad_amd.drainage"]               # (the package's attribute of that name is the function)
av = sys.modules["codecad_amd.assembly_voxels"]
ac = sys.modules["codecad_amd.assembly_components"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hu_drain_layers", "hu_drain_seed", "hu_drain_rise", "hu_drain_floor")
KERNELS = ("k_reach_local<true>", "k_reach_local<false>", "k_reach_merge_faces", "k_reach_merge_all", "k_drain_seed",
           "k_reach_rise<false>", "k_reach_rise<true>", "k_drain_floor<false>", "k_drain_floor<true>")
EVERYTHING = [("scene",) + c for c in CASES] + [("raw",) + c for c in RAW_CASES]


def ref_of(kind, name, axis, up):
    return reference(name, axis, up) if kind == "scene" else raw_reference(name, axis, up)


def labels_of(kind, name, axis):
    return scenes.labels_of(name, axis) if kind == "scene" else scenes.raw_labels(name, axis)


def below(a, axis, up):
    """out[p] = a[the sample below p], False in layer 0."""
    return scenes.shifted(a, axis, 1 if up else -1)


# ---- the references ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,axis,up", EVERYTHING)
def test_the_two_ways_agree_and_the_consequences_hold(kind, name, axis, up):
    ref = ref_of(kind, name, axis, up)
    empty, solid = ref.ids == EMPTY, ref.ids != EMPTY
    assert numpy.array_equal(scenes.layered_escape(empty, axis, up, labels_of(kind, name, axis)), ref.escapes)
    assert numpy.array_equal(ref.trapped, empty & ~ref.escapes) and not (ref.trapped & solid).any()
    # the sample below a trapped sample, and an in-lattice lateral neighbour of it, is solid or trapped
    assert not (ref.trapped & (scenes.layers(ref.ids.shape, axis, up) == 0)).any()
    assert not (ref.trapped & below(ref.escapes, axis, up)).any()
    for a in range(3):
        if a != axis:
            assert not (ref.trapped & (scenes.shifted(ref.escapes, a, 1) | scenes.shifted(ref.escapes, a, -1))).any()
            at = numpy.indices(ref.ids.shape)[a]
            assert not (ref.trapped & ((at == 0) | (at == ref.ids.shape[a] - 1))).any()
    # every trapped sample has a floor, found here by a search down its line
    assert ((ref.trapped_ids != EMPTY) == ref.trapped).all()
    at = numpy.argwhere(ref.trapped)
    for p in at[:: max(1, len(at) // 40)]:
        q, sign = p.copy(), 1 if up else -1
        while True:
            q[axis] -= sign
            assert 0 <= q[axis] < ref.ids.shape[axis], "a trapped sample with no solid below"
            if ref.ids[tuple(q)] != EMPTY:
                break
        assert ref.trapped_ids[tuple(p)] == ref.ids[tuple(q)]
    assert sum(ref.trapped_counts) == int(ref.trapped.sum()) and ((ref.labels == NONE) == ~ref.trapped).all()
    for pool in ref.pools:
        assert set(numpy.unique(ref.trapped_ids[ref.labels == pool.label]).tolist()) == set(pool.parts)


@pytest.mark.parametrize("name", ["hollow_ball", "bell_sealed", "serpentine", "ball_over_slab", "corridor"])
def test_every_sample_of_a_cavity_is_trapped_in_all_six_directions(name):
    ids = scenes.part_ids(name)
    found = comp.reference_components(ids, comp.EMPTY_SPACE)
    sealed = [c for c in found.components if not c.touches_border]
    assert (len(sealed) > 0) == (name in ("hollow_ball", "bell_sealed"))
    inside = numpy.isin(found.labels, [c.label for c in sealed])
    for axis, up in DIRECTIONS:
        ref = reference(name, axis, up)
        assert not (inside & ~ref.trapped).any()
        if name in ("hollow_ball", "bell_sealed"):                                  # ... and nothing else is: the pool IS the cavity
            assert numpy.array_equal(ref.trapped, inside) and len(ref.pools) == 1
            assert (ref.pools[0].label, ref.pools[0].count) == (sealed[0].label, sealed[0].count)


@pytest.mark.parametrize("name", list(MINE))
def test_the_values_by_hand_hold(name):
    sc = SCENES[name]
    assert tuple(int(d) for d in scene(name)[5]) == tuple(sc.frame) == scenes.part_ids(name).shape
    for axis, up in DIRECTIONS:
        ref = reference(name, axis, up)
        if (axis, up) in sc.trapped:
            want = numpy.zeros(ref.ids.shape, dtype=bool)
            for p in sc.trapped[axis, up]:
                want[p] = True
            assert numpy.array_equal(ref.trapped, want), (name, axis, up)
        else:
            assert sc.others == "any" or not ref.trapped.any(), (name, axis, up)


def test_the_cup_and_the_stepped_pocket_by_hand():
    cup = reference("cup", 2, True)
    assert cup.trapped_counts == [6 * 5 * 9] and len(cup.pools) == 1
    pool = cup.pools[0]
    assert (pool.count, pool.box, pool.parts, pool.touches_border) == (270, ((2, 2, 3), (7, 6, 11)), (0,), True)
    assert scenes.level_of(pool, cup.ids.shape, 2, True) == 11 == cup.ids.shape[2] - 1         # the rim is the lattice's top layer
    assert all(not reference("cup", axis, up).trapped.any() for axis, up in DIRECTIONS if (axis, up) != (2, True))
    two = reference("cup_two_parts", 2, True)
    assert two.trapped_counts == [270, 0] and [p.parts for p in two.pools] == [(0,)] and numpy.array_equal(two.trapped, cup.trapped)
    assert set(numpy.unique(two.ids).tolist()) == {0, 1, EMPTY}
    stepped = reference("stepped", 2, True)
    assert stepped.trapped_counts == [5 * 4 * 7, 5 * 4 * 4] and len(stepped.pools) == 1
    pool = stepped.pools[0]
    assert (pool.count, pool.box, pool.parts) == (220, ((1, 1, 3), (10, 4, 9)), (0, 1))
    assert stepped.trapped_ids[3, 2, 9] == 0 and stepped.trapped_ids[8, 2, 9] == 1 and stepped.trapped_ids[8, 2, 5] == EMPTY
    assert scenes.level_of(pool, stepped.ids.shape, 2, True) == 9


def test_the_scenarios_hold_what_they_are_for():
    levels = reference("levels", 2, True)
    assert sorted(scenes.level_of(p, levels.ids.shape, 2, True) for p in levels.pools) == [63, 64, 65]
    assert av.volume_shape(levels.ids.shape, 2 ** 32)[2] == 80 and levels.ids.shape[2] == 70      # ragged: no multiple of 16 or 64
    shaft = reference("shaft", 2, True)
    assert shaft.ids.shape[2] == scenes.NZ == 138 and scenes.NZ % 16 != 0 and scenes.NZ % 64 != 0
    assert shaft.trapped_counts == [135] and (shaft.ids[2, 2, 64:128] == EMPTY).all()       # a word that holds no solid
    assert not reference("shaft", 2, False).trapped.any()
    corridor = reference("corridor", 2, True)
    assert corridor.escapes[7, 4, 64] and corridor.escapes[8, 4, 64] and corridor.escapes[4, 4, 64] and corridor.trapped[4, 4, 63]
    assert [p.count for p in corridor.pools] == [120] and [p.count for p in reference("corridor", 2, False).pools] == [60]
    assert reference("corridor", 0, True).trapped.sum() == 5 * 6 * 7 + 11 and not reference("corridor", 0, False).trapped.any()
    assert not any(reference("bell_gap", axis, up).trapped.any() for axis, up in DIRECTIONS if (axis, up) != (2, False))
    sealed = reference("bell_sealed", 2, True), reference("bell_sealed", 2, False)
    assert [p.parts for p in sealed[0].pools] == [(0,)] and [p.parts for p in sealed[1].pools] == [(1,)]     # the slab; the roof
    assert not any(reference("nothing", axis, up).trapped.any() for axis, up in DIRECTIONS)
    ball = reference("ball_over_slab", 2, True)
    assert len(ball.counts) == 3 and all(c > 0 for c in ball.counts)
    # the serpentine and the U-bend need several handovers: more than one synchronous step
    for name, axis, up in (("serpentine", 0, False), ("serpentine", 2, False), ("u_bend", 2, False), ("corridor", 0, False)):
        empty = scenes.part_ids(name) == EMPTY
        labels = scenes.labels_of(name, axis)
        assert not numpy.array_equal(scenes.synchronous(empty, axis, up, 1, labels), reference(name, axis, up).escapes), (name, axis, up)
    # solid touches the lateral border in every scene of this module
    assert all((scenes.part_ids(name)[0] != EMPTY).any() and (scenes.part_ids(name)[:, 0] != EMPTY).any() for name in MINE)


@pytest.mark.parametrize("kind,name,axis,up", EVERYTHING)
def test_the_synchronous_steps_reach_the_fixed_point_within_n_a(kind, name, axis, up):
    ref = ref_of(kind, name, axis, up)
    empty, labels = ref.ids == EMPTY, labels_of(kind, name, axis)
    na = ref.ids.shape[axis]
    assert numpy.array_equal(scenes.synchronous(empty, axis, up, na, labels), ref.escapes)
    before = scenes.synchronous(empty, axis, up, 0, labels)
    assert not (before & ~ref.escapes).any()
    for k in (1, 2, 3):                                                             # they only grow, inside the fixed point
        now = scenes.synchronous(empty, axis, up, k, labels)
        assert not (before & ~now).any() and not (now & ~ref.escapes).any()
        before = now


@pytest.mark.parametrize("kind,name", sorted({c[:2] for c in EVERYTHING}))
def test_down_an_axis_is_up_the_flipped_volume(kind, name):
    for axis in range(3):
        down = ref_of(kind, name, axis, False)
        n = len(down.counts)
        flipped = scenes.reference_of(numpy.ascontiguousarray(numpy.flip(down.ids, axis)), n, axis, True)
        assert numpy.array_equal(numpy.flip(flipped.trapped_ids, axis), down.trapped_ids)
        assert flipped.trapped_counts == down.trapped_counts and len(flipped.pools) == len(down.pools)


def test_the_layer_labels_are_the_least_index_of_a_layers_component():
    empty = numpy.zeros((2, 3, 2), dtype=bool)
    empty[0, :, 0] = True                                                           # a run along y in the plane z = 0 ...
    empty[0, 1, 1] = empty[1, 1, 1] = True                                          # ... and a pair along x in the plane z = 1
    along_z = scenes.layer_labels(empty, 2)
    assert along_z[0, :, 0].tolist() == [0, 0, 0] and along_z[0, 1, 1] == along_z[1, 1, 1] == 3 and along_z[1, 0, 0] == NONE
    along_x = scenes.layer_labels(empty, 0)
    assert along_x[0, :, 0].tolist() == [0, 0, 0] and along_x[0, 1, 1] == 0 and along_x[1, 1, 1] == 9     # joined along z within x = 0
    along_y = scenes.layer_labels(empty, 1)
    assert along_y[0, :, 0].tolist() == [0, 2, 4] and along_y[0, 1, 1] == 2 and along_y[1, 1, 1] == 2


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_refusals():
    one = cc.assembly("one", [shapes.sphere(r=1).make_part("ball")])
    with pytest.raises(ValueError):
        cc.drainage(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1)
    with pytest.raises(ValueError):
        cc.drainage(one, -1)
    for bad in (3, -1, True, None, "z", 2.0):
        with pytest.raises(ValueError, match="axis"):
            cc.drainage(one, 0.125, axis=bad)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.drainage(one, 0.125, max_bytes=6 * 16 * 16 * 16 - 1)
    with pytest.raises(ValueError, match="64"):
        cc.drainage(cc.assembly("many", [shapes.box(1).make_part("b%d" % k).translated_x(2 * k) for k in range(65)]), 0.5)
    assert {"drainage", "DrainageReport", "Pool"} <= set(cc.__all__) and "drainage(" in cc.__doc__ and dr.SAMPLE_BYTES == 6
    assert dr.DrainageReport._fields == ("instances", "corner", "step", "dims", "axis", "up", "part_ids", "trapped_ids", "trapped_counts",
                                         "trapped_volume", "pools", "labels", "passes", "samples_evaluated", "traversals",
                                         "component_capacity_runs")
    for word in ("ESCAPE", "TRAPPED", "FLOOR", "POOLS", "THE TOP FACE IS NO EXIT", "THE OUTSIDE IS A SINK", "OUT OF SCOPE", "grounded",
                 "partial fill", "thin_walls", "more than 64 instances", "several devices"):
        assert word in dr.__doc__, word


def test_no_visible_instance_gives_the_empty_report():
    report = cc.drainage(dis_scenes.empty_assembly(), 0.1, axis=0, up=False, max_bytes=6 * 16)
    assert report.instances == [] and report.traversals == 0 and report.samples_evaluated == 0 and report.passes == 0
    assert report.part_ids.shape == (1, 1, 1) == report.trapped_ids.shape == report.labels.shape and (report.axis, report.up) == (0, False)
    assert report.trapped_ids[0, 0, 0] == 255 and report.trapped_ids.dtype == numpy.uint8
    assert report.labels[0, 0, 0] == NONE and report.labels.dtype == numpy.uint32
    assert report.trapped_counts == [] and report.trapped_volume == 0.0 and report.pools == [] and report.component_capacity_runs == 0
    assert report.drains
    with pytest.raises(ValueError):
        cc.drainage(dis_scenes.empty_assembly(), 0.1, max_bytes=6 * 16 - 1)


def fake_device(monkeypatch, changed, counts):
    """drainage() over a library that records its calls; the changed word reads as the values of `changed` in turn."""
    calls, words = [], list(changed)

    class Buffer:
        def __init__(self, dtype, shape, queue=None):
            self.dtype, self.shape = numpy.dtype(dtype), tuple(shape)
            self.size = int(numpy.prod(shape)) * self.dtype.itemsize
            self.device_ptr = 0x100000 * (1 + len([c for c in calls if c[0] == "buffer"]))
            calls.append(("buffer", self.dtype, self.shape))

        def read(self):
            calls.append(("read", self.device_ptr, self.size))
            if self.dtype == ac._ROW:
                return numpy.zeros(self.shape, self.dtype)                          # the counter reads 0: no pool
            if self.shape == (1,):
                return numpy.array([words.pop(0)], dtype=numpy.uint32)
            return counts.copy() if self.dtype == numpy.uint64 else numpy.full(self.shape, 1, self.dtype)

        def release(self):
            calls.append(("release", self.device_ptr))

    class Lib:
        def __getattr__(self, name):
            def call(*args):
                calls.append((name, args))
                return 0
            return call

    def traverse(inst, top, side, c, s, d, initial_capacity, **kwargs):
        calls.append(("traverse", initial_capacity, kwargs["cells_extra"][0]))
        return 77, numpy.array([5, 6, 7, 999], dtype=numpy.uint64), 2

    manager = types.SimpleNamespace(lib=Lib(), queue=types.SimpleNamespace(handle=0x99))
    for module in (av, ac, dr):
        monkeypatch.setattr(module, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


@pytest.mark.parametrize("axis,up", [(2, True), (0, False)])
def test_the_driver_reads_one_word_a_pass_and_labels_the_trapped_ids(monkeypatch, axis, up):
    asm, resolution = dis_scenes.scene("hooks")[:2]
    counts = numpy.arange(100, 164, dtype=numpy.uint64)
    calls = fake_device(monkeypatch, [1, 1, 0], counts)
    report = cc.drainage(asm, resolution, axis=axis, up=up, local=False, initial_capacity=7, initial_components=3, max_bytes=6 * 14 * 10 * 144)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    assert names[:4] == ["buffer", "hu_memset", "traverse", "read"]                 # the ids, as assembly_voxels() leaves them
    assert names[4:11] == ["buffer", "hu_memset", "buffer", "buffer", "hu_drain_layers", "hu_components_flatten", "hu_drain_seed"]
    assert names[11:20] == ["hu_memset", "hu_drain_rise", "read"] * 3               # three passes: the third sets nothing
    assert names[20:28] == ["buffer", "hu_drain_floor", "read", "read", "release", "release", "release", "release"]
    assert names[28:] == ["buffer", "hu_components_local", "hu_components_merge", "hu_components_flatten", "buffer", "hu_memset",
                          "hu_components_stats", "read", "release", "release", "hu_components_finish", "read", "release"]
    assert "hu_stream_synchronize" not in names and calls[2][1:] == (7, 1)
    ids, acc, word, layers, trapped = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    assert calls[4][1:] == (numpy.dtype(numpy.uint64), (64,)) and calls[5][1] == (acc, 0, 512, 0x99)
    assert calls[6][1:] == (numpy.dtype(numpy.uint32), (1,)) and calls[7][1:] == (numpy.dtype(numpy.uint32), (14, 10, 144))
    launch = calls[8][1]
    assert launch[:2] + launch[3:] == (ids, layers, 144, axis, 0, 0x99) and list(launch[2]) == [14, 10, 138]
    assert calls[9][1][0] == layers and calls[10][1][:1] + calls[10][1][2:] == (layers, 144, axis, int(up), 0x99)
    for k in range(3):
        assert calls[11 + 3 * k][1] == (word, 0, 4, 0x99)
        rise = calls[12 + 3 * k][1]
        assert rise[:2] + rise[3:] == (layers, word, 144, axis, int(up), 0x99)
        assert calls[13 + 3 * k] == ("read", word, 4)                               # four bytes a pass
    floor = calls[21][1]
    assert calls[20][1:] == (numpy.dtype(numpy.uint8), (14, 10, 144))
    assert floor[:4] + floor[5:] == (ids, layers, trapped, acc, 144, axis, int(up), 0x99)
    assert [c[1] for c in calls[22:28]] == [trapped, acc, layers, ids, acc, word]   # one read-back, then everything but the trapped ids goes
    assert calls[29][1][0] == trapped and calls[29][1][4:6] == (1, 0)               # the trapped ids are labelled: solid, the same arm
    assert calls[37] == ("release", trapped)
    assert report.passes == 3 and report.trapped_counts == [100, 101, 102] and all(type(v) is int for v in report.trapped_counts)
    assert report.trapped_volume == 303 * float(report.step) ** 3 and (report.axis, report.up) == (axis, up)
    assert report.part_ids.shape == (14, 10, 138) == report.trapped_ids.shape == report.labels.shape
    assert report.pools == [] and report.component_capacity_runs == 1 and report.traversals == 2 and report.samples_evaluated == 77


def test_max_bytes_counts_six_bytes_a_sample_before_any_launch(monkeypatch):
    asm, resolution = dis_scenes.scene("hooks")[:2]
    calls = fake_device(monkeypatch, [0], numpy.zeros(64, numpy.uint64))
    with pytest.raises(ValueError, match="max_bytes"):
        cc.drainage(asm, resolution, max_bytes=6 * 14 * 10 * 144 - 1)
    with pytest.raises(ValueError, match="axis"):
        cc.drainage(asm, resolution, axis=3)
    with monkeypatch.context() as m:
        m.setattr(dr, "_check_entries", lambda dims: (_ for _ in ()).throw(ValueError("entries")))
        with pytest.raises(ValueError, match="entries"):
            cc.drainage(asm, resolution)
    with pytest.raises(ValueError, match="2\\^31"):
        ac._check_entries((65536, 32768, 1))                                        # 2^31 * 16 entries under the padding
    assert calls == []
    cc.drainage(dis_scenes.empty_assembly(), 0.1)
    assert calls == []                                                              # nothing visible: nothing launched


def test_a_pool_takes_its_names_and_its_level_from_its_row():
    voxels = types.SimpleNamespace(instances=[types.SimpleNamespace(name="a"), types.SimpleNamespace(name="b")], corner=(0.0, 0.0, 0.0),
                                   step=numpy.float32(0.5), dims=(10, 20, 30))
    rows = numpy.zeros(1, ac._ROW)
    rows[0] = (4, (8, 12, 16), 0b10, (~numpy.uint32(1), ~numpy.uint32(2), ~numpy.uint32(3)), (4, 5, 6), 77, 0)
    for axis, up, level in ((2, True, 6), (2, False, 26), (0, True, 4), (0, False, 8), (1, False, 17)):
        (pool,) = dr._pools(rows, voxels, axis, up)
        assert (pool.label, pool.count, pool.box, pool.parts, pool.held_by, pool.level) == (77, 4, ((1, 2, 3), (4, 5, 6)), (1,), ("b",), level)
        assert pool.volume == 4 * 0.125 and tuple(pool.centroid) == (1.0, 1.5, 2.0)


# ---- the C ABI, the entry points' refusals and the kernels' resources --------------------------------------------------

def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    with open(_lib.HEADER) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    want = {"hu_drain_layers": ["const void* ids_dev", "void* labels_dev", "const uint32_t dims[3]", "uint32_t pitch", "int axis", "int local",
                                "void* stream"],
            "hu_drain_seed": ["void* labels_dev", "const uint32_t dims[3]", "uint32_t pitch", "int axis", "int up", "void* stream"],
            "hu_drain_rise": ["void* labels_dev", "uint32_t* changed_dev", "const uint32_t dims[3]", "uint32_t pitch", "int axis", "int up",
                              "void* stream"],
            "hu_drain_floor": ["const void* ids_dev", "const void* labels_dev", "void* trapped_dev", "uint64_t* counts_dev",
                               "const uint32_t dims[3]", "uint32_t pitch", "int axis", "int up", "void* stream"]}
    assert tuple(want) == ENTRY_POINTS
    for name, args in want.items():
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert [" ".join(a.split()) for a in proto.split(",")] == args
        assert len(_lib.PROTOTYPES[name]) == len(args)
        dims = args.index("const uint32_t dims[3]")
        assert _lib.PROTOTYPES[name][dims] is _lib.PROTOTYPES["hu_components_flatten"][1] and _lib.PROTOTYPES[name][dims + 1] is ctypes.c_uint32
        assert ("int %s(" % name) in integration
    assert int(re.search(r"#define HU_ABI_VERSION (\d+)", header).group(1)) == 3 == lib.hu_abi_version()    # additive: the version stayed


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    d = lambda *v: (ctypes.c_uint32 * 3)(*v)                                          # noqa: E731
    p = 0x1000                                                                        # never dereferenced: every call is refused

    def layers(ids=p, labels=p, dims=d(4, 4, 4), pitch=16, axis=2):
        return lib.hu_drain_layers(ids, labels, dims, pitch, axis, 1, None)

    def seed(labels=p, dims=d(4, 4, 4), pitch=16, axis=2):
        return lib.hu_drain_seed(labels, dims, pitch, axis, 1, None)

    def rise(labels=p, word=p, dims=d(4, 4, 4), pitch=16, axis=2):
        return lib.hu_drain_rise(labels, word, dims, pitch, axis, 1, None)

    def floor(ids=p, labels=p, trapped=p, counts=p, dims=d(4, 4, 4), pitch=16, axis=2):
        return lib.hu_drain_floor(ids, labels, trapped, counts, dims, pitch, axis, 1, None)

    refused = [layers(ids=None), layers(labels=None), layers(dims=None), seed(labels=None), seed(dims=None), rise(labels=None), rise(word=None),
               rise(dims=None), floor(ids=None), floor(labels=None), floor(trapped=None), floor(counts=None), floor(dims=None)]
    refused += [f(axis=bad) for f in (layers, seed, rise, floor) for bad in (3, -1)]
    refused += [f(pitch=bad) for f in (layers, seed, rise, floor) for bad in (24, 0, 8)]
    refused += [f(dims=bad) for f in (layers, seed, rise, floor) for bad in (d(4, 4, 17), d(0, 4, 4), d(4, 0, 4), d(4, 4, 0), d(65537, 4, 4))]
    refused += [layers(ids=p + 8), layers(ids=p + 1), layers(labels=p + 2), seed(labels=p + 1), rise(labels=p + 2), rise(word=p + 2),
                floor(labels=p + 2), floor(counts=p + 4)]
    big = d(65536, 32768, 1)                                                          # 2^31 lines of pitch 16: 2^35 entries
    refused += [layers(dims=big), seed(dims=big), rise(dims=big), floor(dims=big), seed(dims=d(65536, 32768, 17), pitch=32),
                seed(dims=d(32768, 4097, 16))]
    assert refused == [-3] * len(refused)
    assert seed(dims=big) == -3 and b"2^31" in lib.hu_last_error()
    assert rise(axis=3) == -3 and b"axis" in lib.hu_last_error()
    assert floor(pitch=24) == -3 and b"16" in lib.hu_last_error()
    assert layers(ids=p + 8) == -3 and b"aligned" in lib.hu_last_error()
    assert floor(counts=p + 4) == -3 and b"aligned" in lib.hu_last_error()
    assert rise(word=None) == -3 and b"NULL" in lib.hu_last_error()


def test_the_kernels_use_no_scratch_and_the_resources_the_design_states():
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, and the VGPR counts and
    the LDS written in DESIGN.md; LDS in the tile kernel alone; every kernel of the unit is held to section 9.2 or 9.3."""
    from codecad_amd.hip_util import builder
    assert reach.UNIT in builder.SOURCES and reach.UNIT not in builder.FLAGGED_SOURCES
    everything = reach.sources()
    for gone in ("instance_drain.hip", "instance_ground.hip"):
        assert gone not in builder.SOURCES and gone not in everything
    source, shared, labelling, components = (everything[name] for name in (reach.UNIT, "id_volume.hpp", "label_kernels.hpp",
                                                                           "instance_components.hip"))
    assert '#include "id_volume.hpp"' in source and '#include "label_kernels.hpp"' in source
    assert '#include "id_volume.hpp"' in labelling and '#include "label_kernels.hpp"' in components
    # one copy of each: find, unite and the line walk in id_volume.hpp; the tile labelling, the merges, the tile's index
    # arithmetic and the grid of a lane per sample in label_kernels.hpp; nothing of them in either unit
    for home, text, functions in (("id_volume.hpp", shared, ("uint32_t find(", "void unite(", "LineUnitOf<I> line_unit(", "uint64_t line_units(")),
                                  ("label_kernels.hpp", labelling, ("void label_tile(", "void label_merge_faces(", "void label_merge_all(",
                                                                    "uint32_t blocks_of(", "uint64_t face_pairs(", "int labels_of(",
                                                                    "constexpr uint32_t kNone = 0xffffffffu", "constexpr uint32_t kTileX",
                                                                    "__shared__ uint32_t lab[kTile]"))):
        for function in functions:
            assert text.count(function) == 1, function
            assert [name for name, other in everything.items() if function in other] == [home], function
    for text in (source, components):                                              # no tile arithmetic, no face ranges
        assert "kTileX" not in text and "kTileZ" not in text and "line * a.segments" not in text and "2^31 entries\"" not in text
    # the unit wraps the one labelling body once: one stage-1 kernel set for every predicate
    for wrapped in ("label_tile<", "label_merge_faces(", "label_merge_all("):
        assert source.count(wrapped) == 1, wrapped
    assert [name for name, other in everything.items() if "k_drain_" in other] == [reach.UNIT]
    documented = reach.documented_resources(KERNELS)
    found = reach.compiled_resources()
    if found is None:
        pytest.skip("no hipcc in this environment")
    assert set(found) == set(reach.DRAIN) | set(reach.GROUND) and len(found) == 12
    assert all(private == 0 for _, _, private in found.values()), found
    assert {k: v[:2] for k, v in found.items() if k in KERNELS} == documented
    assert {k for k, (_, lds, _) in found.items() if lds} == {"k_reach_local<true>", "k_reach_local<false>"}
    assert found["k_reach_local<true>"][1] == 4096 + 256
