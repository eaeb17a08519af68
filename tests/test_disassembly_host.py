"""The reference and the scenarios of test_gpu_disassembly.py, and the host side of disassembly(), checked without a device.

disassembly_scenes.reference_blocking is written from the definition: for t = 1, 2, ... the first t at which part i moved by t
steps meets part j.  That a walk up every line with a running last index per part gives the same matrices and witnesses on
every scenario, and that both give the values written by hand, is the first test.  Every scenario names the entries it exists
for.  Then the report's methods, the driver over a recording library, the C ABI, the entry point's refusals and the kernels'
resources."""
import ctypes
import math
import os
import re
import subprocess
import sys
import types

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes
from codecad_amd.hip_util import _lib

import disassembly_scenes as scenes
from disassembly_scenes import SCENES, NAMES, NEVER, reference, scene, NZ

dis = sys.modules["codecad_amd.disassembly"]           # (the package's attribute of that name is the function)
av = sys.modules["codecad_amd.assembly_voxels"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_block_lines", "k_block_columns")


def report_of(name):
    """A DisassemblyReport over the reference of a scene: the methods are plain host code on the two arrays."""
    asm, resolution, instances, corner, step, dims = scene(name)
    ref = reference(name)
    return dis.DisassemblyReport(list(instances), corner, step, dims, ref.ids, ref.counts, ref.distance, ref.witness, 0, 1)


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_a_line_by_hand():
    """One line along x: 0 0 . 1 1 0 . 2 -- the later sample of 0 counts for 2, the earlier one for 1."""
    ids = numpy.array([0, 0, 255, 1, 1, 0, 255, 2], dtype=numpy.uint8).reshape(8, 1, 1)
    for way in (scenes.reference_blocking, scenes.running_blocking):
        distance, witness = way(ids, 3)
        assert distance[0].tolist() == [[NEVER, 2, 2], [1, NEVER, 3], [NEVER, NEVER, NEVER]]
        assert witness[0, 0, 1].tolist() == [1, 0, 0] and witness[0, 0, 2].tolist() == [5, 0, 0] and witness[0, 1, 0].tolist() == [4, 0, 0]
        assert witness[0, 1, 2].tolist() == [4, 0, 0] and witness[0, 2, 0].tolist() == [-1, -1, -1]
        assert (distance[1:] == NEVER).all() and (witness[1:] == -1).all()
    assert scenes.reference_order(distance) == ([(0, 1, True), (1, 0, False), (2, 0, True)], [])
    assert dis.NEVER == NEVER == 0xffffffff and dis.MAX_PARTS == 64 and list(dis.DIRECTIONS) == scenes.DIRECTIONS


@pytest.mark.parametrize("name", NAMES)
def test_the_two_ways_and_the_values_by_hand_agree(name):
    sc, ref = SCENES[name], reference(name)
    n = len(ref.counts)
    assert tuple(int(d) for d in scene(name)[5]) == tuple(sc.frame) == ref.ids.shape
    distance, witness = scenes.running_blocking(ref.ids, n)
    assert numpy.array_equal(distance, ref.distance) and numpy.array_equal(witness, ref.witness)
    assert distance.dtype == ref.distance.dtype == numpy.uint32 and witness.dtype == ref.witness.dtype == numpy.int32
    for (axis, i, j), (d, p) in sc.by_hand.items():
        assert (int(ref.distance[axis, i, j]), tuple(ref.witness[axis, i, j].tolist())) == (d, tuple(p)), (axis, i, j)
    finite = ref.distance != NEVER
    assert ((ref.witness == -1).all(axis=-1) == ~finite).all() and not finite[:, numpy.arange(n), numpy.arange(n)].any()
    at = numpy.argwhere(finite)
    for axis, i, j in at[:: max(1, len(at) // 50)]:                                 # a witness is a sample of i with one of j D beyond
        p = ref.witness[axis, i, j].copy()
        assert ref.ids[tuple(p)] == i
        p[axis] += ref.distance[axis, i, j]
        assert ref.ids[tuple(p)] == j


@pytest.mark.parametrize("name", NAMES)
def test_no_scenario_is_vacuous(name):
    """Every scenario names the entries it exists for: finite ones, with their values, and ones that must be NEVER."""
    sc, ref = SCENES[name], reference(name)
    assert sc.by_hand or name == "single"
    assert all(ref.distance[key] != NEVER for key in sc.by_hand) and all(ref.distance[key] == NEVER for key in sc.never)
    assert len(sc.never) > 0 or name.startswith("again")
    assert all(c > 0 for c in ref.counts)
    if sc.order is not None:
        assert scenes.reference_order(ref.distance) == sc.order
    if sc.frame[2] == NZ:
        assert av.volume_shape(sc.frame, 2 ** 32)[2] == 144 > NZ == 138


def test_the_scenarios_hold_what_they_are_for():
    peg = reference("peg").distance
    assert peg[2, 0, 1] == NEVER and peg[2, 1, 0] == 1 and (peg[:2, [0, 1], [1, 0]] == 1).all()
    between = reference("between_x").distance[0]
    assert between[0, 2] == between[0, 1] + 2 + between[1, 2]                       # across the three samples of k
    for name, axis in (("again_x", 0), ("again_z", 2)):
        d = reference(name).distance[axis]
        assert NEVER != d[0, 1] != d[1, 0] != NEVER
    words = reference("words")
    assert words.distance[2, 5, 6] == 11 and words.ids[2, 0, 60:70].tolist() == [5] * 10      # the run across 63 | 64 ended at 69
    assert words.ids[3, 0, 62:66].tolist() == [255, 8, 8, 255] and words.ids[4, 0, 63] == 255 and words.ids[4, 0, 64] == 11
    assert (words.ids[5, :, 64:128] == 255).all() and (words.ids[6, 0, 128:] == numpy.array([14] * 2 + [255] * 6 + [15] * 2)).all()
    for name, axis in (("slabs64_x", 0), ("slabs64_z", 2)):
        ref = reference(name)
        i, j = numpy.indices((64, 64))
        assert numpy.array_equal(ref.distance[axis], numpy.where(j > i, 2 * (j - i) - 1, NEVER))
        assert ref.counts == [32] * 64 and ref.distance[axis, 0, 63] == 125 and ref.distance[axis, 62, 63] == 1
        other = [a for a in range(3) if a != axis]
        assert (ref.witness[axis][j > i][:, other] == 0).all()                     # a tie across 16 lines: the first line wins
    ball = reference("ownership")
    assert (ball.ids == 0).sum() == 4 ** 3 and ball.distance[2, 2, 0] == 99         # the cap owns the ball's lowest samples
    assert ball.distance[2, 2, 1] > 99 - 4                                          # ... so the ball itself lies further above the slab
    hooks = reference("hooks").distance
    assert (hooks[:, [0, 1], [1, 0]] != NEVER).all()                                # each link blocks the other both ways on every axis
    for name, axis in (("long_x", 0), ("long_z", 2)):
        ref = reference(name)
        assert ref.distance[axis, 0, 2] == 40002 > 32767 and ref.witness[axis, 1, 2, axis] == 40003 > 32767
        assert ref.ids.size == 40010 * 16 and av.volume_shape(ref.ids.shape, 2 ** 32)[2] % 16 == 0


@pytest.mark.parametrize("name", NAMES)
def test_downwards_is_the_transpose(name):
    """The distance from i to j along -a is D_a[j][i]: the matrices of the ids flipped along a are the transposes."""
    ref = reference(name)
    n = len(ref.counts)
    for axis in range(3):
        flipped = scenes.running_blocking(numpy.flip(ref.ids, axis), n)[0] if n > 16 or ref.ids.size > 10 ** 5 else \
            scenes.reference_blocking(numpy.ascontiguousarray(numpy.flip(ref.ids, axis)), n)[0]
        assert numpy.array_equal(flipped[axis], ref.distance[axis].T)
        for other in range(3):
            if other != axis:
                assert numpy.array_equal(flipped[other], ref.distance[other])


# ---- the report's methods ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_order_follows_the_rule(name):
    report, ref, sc = report_of(name), reference(name), SCENES[name]
    got = report.order()
    assert got == scenes.reference_order(ref.distance) and (sc.order is None or got == sc.order)
    sequence, stuck = got
    assert sorted([k for k, _, _ in sequence] + stuck) == list(range(len(ref.counts)))
    rest = list(range(len(ref.counts)))
    for k, axis, up in sequence:                                                    # each move is free among what is left
        assert report.blockers(k, axis, up, among=rest) == [] and (axis, up) == report.free_directions(k, among=rest)[0]
        assert all(not report.free_directions(lower, among=rest) for lower in rest if lower < k)
        rest.remove(k)
    assert rest == stuck and all(report.free_directions(k, among=stuck) == [] for k in stuck) and len(stuck) != 1


def test_steps_travel_and_contacts():
    peg = report_of("peg")
    step = float(peg.step)
    assert peg.steps(0, 1, 2, True) == NEVER and peg.steps(0, 1, 2, False) == 1 and type(peg.steps(0, 1, 2, False)) is int
    assert peg.travel(0, 2, True) == math.inf and peg.travel(0, 2, False) == 0.0 and peg.travel(0, 0, True) == 0.0
    assert peg.free_directions(0) == [(2, True)] and peg.free_directions(1) == [(2, False)]
    assert peg.contacts(2) == [(1, 0)] and peg.contacts(0) == [(0, 1), (1, 0)] == peg.contacts(1)
    assert peg.order() == ([(0, 2, True), (1, 0, True)], [])
    between = report_of("between_x")
    assert between.blockers(0, 0, True) == [1, 2] and between.blockers(0, 0, False) == [] and between.blockers(2, 0, False) == [0, 1]
    assert between.travel(0, 0, True) == 2 * step and between.travel(0, 0, True, among=[0, 2]) == 9 * step
    assert between.travel(2, 0, False) == 4 * step and between.travel(1, 0, True, among=(1,)) == math.inf
    assert between.steps(2, 0, 0, False) == 10 and between.steps(2, 0, 0, True) == NEVER
    apart = report_of("apart_z")
    assert apart.travel(0, 2, True) == 60 * float(apart.step) and apart.contacts(2) == []


def test_a_group_is_blocked_by_what_is_outside_it():
    hooks = report_of("hooks")
    assert hooks.free_directions(0) == [] == hooks.free_directions(1) and hooks.free_directions(0, among=[0, 2]) != []
    assert hooks.blockers((0, 1), 0, True) == [2] and hooks.blockers(iter([1, 0]), 0, False) == []
    assert hooks.free_directions([0, 1]) == [d for d in scenes.DIRECTIONS if d != (0, True)]
    assert hooks.free_directions([0, 1], among=[0, 1]) == scenes.DIRECTIONS == hooks.free_directions([0, 1, 2])
    assert hooks.blockers(numpy.int64(0), 2, True) == [1] and hooks.blockers(0, 2, True, among=[2]) == []
    assert hooks.order() == ([(2, 0, True)], [0, 1])


def test_the_methods_refuse_what_is_no_part_or_axis():
    peg = report_of("peg")
    for bad in (2, -1, True, 0.0, "0", None, [0, 2], [0.5]):
        with pytest.raises(ValueError):
            peg.blockers(bad, 0, True)
        if bad is not None:                                                         # (among=None is everything)
            with pytest.raises(ValueError):
                peg.free_directions(0, among=bad)
    for bad in (3, -1, True, None, "x", 1.0):
        with pytest.raises(ValueError, match="axis"):
            peg.steps(0, 1, bad, True)
        with pytest.raises(ValueError, match="axis"):
            peg.contacts(bad)
    with pytest.raises(ValueError):
        peg.steps(0, 2, 0, True)
    with pytest.raises(ValueError):
        peg.travel([0, 1], 0, True)


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_refusals():
    one = cc.assembly("one", [shapes.sphere(r=1).make_part("ball")])
    with pytest.raises(ValueError):
        cc.disassembly(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1)
    with pytest.raises(ValueError):
        cc.disassembly(one, -1)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.disassembly(one, 0.125, max_bytes=16 * 16 * 16 - 1)
    with pytest.raises(ValueError, match="64"):
        cc.disassembly(cc.assembly("many", [shapes.box(1).make_part("b%d" % k).translated_x(2 * k) for k in range(65)]), 0.5)
    with pytest.raises(ValueError):
        cc.disassembly(cc.assembly("long", [shapes.box(70000 * 0.01, 0.1, 0.1).make_part("rod")]), 0.01)
    assert {"disassembly", "DisassemblyReport"} <= set(cc.__all__) and "disassembly(" in cc.__doc__


def test_no_visible_instance_gives_the_empty_report():
    report = cc.disassembly(scenes.empty_assembly(), 0.1, max_bytes=16)
    assert report.instances == [] and report.counts == [] and report.traversals == 0 and report.samples_evaluated == 0
    assert report.distance.shape == (3, 0, 0) and report.distance.dtype == numpy.uint32
    assert report.witness.shape == (3, 0, 0, 3) and report.witness.dtype == numpy.int32
    assert report.part_ids.shape == (1, 1, 1) and report.part_ids[0, 0, 0] == 255
    assert report.order() == ([], []) and report.contacts(0) == []
    with pytest.raises(ValueError):
        cc.disassembly(scenes.empty_assembly(), 0.1, max_bytes=15)


def fake_device(monkeypatch, table):
    """disassembly() over a library that records its calls and a key table that reads back as `table`."""
    calls = []

    class Buffer:
        def __init__(self, dtype, shape, queue=None):
            self.dtype, self.shape = numpy.dtype(dtype), tuple(shape)
            self.size = int(numpy.prod(shape)) * self.dtype.itemsize
            self.device_ptr = 0x100000 * (1 + len([c for c in calls if c[0] == "buffer"]))
            calls.append(("buffer", self.dtype, self.shape))

        def read(self):
            calls.append(("read", self.device_ptr))
            return table.copy() if self.dtype == numpy.uint64 else numpy.full(self.shape, 1, self.dtype)

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
    for module in (av, dis):
        monkeypatch.setattr(module, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


def test_the_driver_sets_the_table_once_and_launches_once_per_axis(monkeypatch):
    asm, resolution = scene("hooks")[:2]
    table = numpy.full((3, 64, 64), 0xffffffffffffffff, dtype=numpy.uint64)
    table[0, 0, 1] = 3 << 48 | 1 << 32 | 4 << 16 | 60
    table[2, 2, 0] = 40001 << 48 | 65535 << 32 | 40000 << 16 | 7
    table[1, 5, 6] = 1                                                              # beyond n = 3: never looked at
    calls = fake_device(monkeypatch, table)
    report = cc.disassembly(asm, resolution, initial_capacity=7, max_bytes=14 * 10 * 144)
    monkeypatch.undo()
    assert [c[0] for c in calls] == ["buffer", "hu_memset", "traverse", "read",     # the ids, as assembly_voxels() leaves them
                                     "buffer", "hu_memset", "hu_blocking_lines", "hu_blocking_lines", "hu_blocking_lines",
                                     "read", "release", "release"]
    assert calls[2][1:] == (7, 1)                                                   # retire=True, the cell lists' capacity
    ids, keys = 0x100000, 0x200000
    assert calls[4][1:] == (numpy.dtype(numpy.uint64), (3, 64, 64)) and calls[5][1] == (keys, 0xff, 3 * 64 * 64 * 8, 0x99)
    for axis, call in enumerate(calls[6:9]):
        #      ids, keys | pitch, axis, n, stream
        assert call[1][:2] + call[1][3:] == (ids, keys, 144, axis, 3, 0x99) and list(call[1][2]) == [14, 10, 138]
    assert calls[9] == ("read", keys) and [c[1] for c in calls[10:]] == [ids, keys]
    assert report.distance.shape == (3, 3, 3) and report.distance[0, 0, 1] == 3 and report.distance[2, 2, 0] == 40001
    assert (report.distance != NEVER).sum() == 2 and report.distance.dtype == numpy.uint32 and report.witness.dtype == numpy.int32
    assert report.witness[0, 0, 1].tolist() == [1, 4, 60] and report.witness[2, 2, 0].tolist() == [65535, 40000, 7]
    assert (report.witness[report.distance == NEVER] == -1).all()
    assert report.counts == [5, 6, 7] and report.traversals == 2 and report.samples_evaluated == 77
    assert report.part_ids.shape == (14, 10, 138) and len(report.instances) == 3


def test_max_bytes_counts_one_byte_a_sample_before_any_launch(monkeypatch):
    asm, resolution = scene("hooks")[:2]
    calls = fake_device(monkeypatch, numpy.zeros((3, 64, 64), numpy.uint64))
    with pytest.raises(ValueError, match="max_bytes"):
        cc.disassembly(asm, resolution, max_bytes=14 * 10 * 144 - 1)
    assert calls == []
    cc.disassembly(scenes.empty_assembly(), 0.1)
    assert calls == []                                                              # nothing visible: nothing launched


# ---- the C ABI, the entry point's refusals and the kernels' resources -------------------------------------------------

def test_abi_of_the_new_entry_point():
    lib = _lib.load()
    with open(_lib.HEADER) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    name = "hu_blocking_lines"
    assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    assert [" ".join(a.split()) for a in proto.split(",")] == ["const void* ids_dev", "uint64_t* keys_dev", "const uint32_t dims[3]",
                                                              "uint32_t pitch", "int axis", "uint32_t n", "void* stream"]
    assert len(_lib.PROTOTYPES[name]) == 7 and _lib.PROTOTYPES[name][2] is _lib.PROTOTYPES["hu_overhang_mark"][4]     # dims
    assert _lib.PROTOTYPES[name][4] is ctypes.c_int and _lib.PROTOTYPES[name][5] is ctypes.c_uint32
    assert ("int %s(" % name) in integration
    assert int(re.search(r"#define HU_BLOCKING_MAX_PARTS (\d+)", header).group(1)) == dis.MAX_PARTS == dis._KEYS[1] == dis._KEYS[2]


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    d = lambda *v: (ctypes.c_uint32 * 3)(*v)                                          # noqa: E731
    p = 0x1000                                                                        # never dereferenced: every call is refused

    def lines(ids=p, keys=p, dims=d(4, 4, 4), pitch=16, axis=0, n=2):
        return lib.hu_blocking_lines(ids, keys, dims, pitch, axis, n, None)

    refused = [lines(ids=None), lines(keys=None), lines(dims=None), lines(keys=p + 4), lines(keys=p + 1), lines(pitch=24), lines(pitch=0),
               lines(pitch=8), lines(dims=d(4, 4, 17)), lines(dims=d(0, 4, 4)), lines(dims=d(4, 0, 4)), lines(dims=d(4, 4, 0)),
               lines(dims=d(65537, 4, 4)), lines(dims=d(4, 65537, 4)), lines(axis=3), lines(axis=-1), lines(n=0), lines(n=65),
               lines(axis=2, n=0), lines(axis=2, pitch=20), lines(axis=1, keys=None)]
    assert refused == [-3] * len(refused)
    assert lines(n=65) == -3 and b"n must" in lib.hu_last_error()
    assert lines(axis=3) == -3 and b"axis" in lib.hu_last_error()
    assert lines(pitch=24) == -3 and b"16" in lib.hu_last_error()
    assert lines(keys=p + 4) == -3 and b"aligned" in lib.hu_last_error()


def documented_resources():
    """{kernel: (VGPRs, LDS bytes)} as DESIGN.md states them."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    found = {}
    for name in KERNELS:
        m = re.search(r"`%s` (\d+) VGPRs and (\d+) B of LDS" % re.escape(name), text)
        assert m, "DESIGN.md section 9 states the VGPRs and the LDS of " + name
        found[name] = (int(m.group(1)), int(m.group(2)))
    return found


def test_the_kernels_use_no_scratch_and_the_resources_the_design_states(tmp_path):
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, no LDS of a fixed size
    (the key table and the last indices are sized by n at the launch) and the VGPR counts written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_blocking.hip" in builder.SOURCES and "instance_blocking.hip" not in builder.FLAGGED_SOURCES
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_blocking.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_blocking.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"\d+(k_block_lines|k_block_columns)ENS_9BlockArgsE", name)
        assert m, name
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        found[m.group(1)] = (int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1)),
                             int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)))
    assert found == documented_resources()
    assert all(lds == 0 for _, lds in found.values())
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "n * n * 8 + n * 512" in f.read()                                    # what the launch asks for, at most 64 KiB
