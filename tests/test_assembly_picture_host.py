"""The picture of an assembly (codecad_amd/rendering/assembly_picture.py), the parts that need no device: which instances
get an id, their colours, every ValueError, the camera it shares with `asm.shape()`, and the C ABI of its entry points."""
import collections
import ctypes
import os
import re
import subprocess

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, rendering
from codecad_amd.rendering import assembly_picture as ap, ray_caster
from codecad_amd.hip_util import _lib


def _assembly():
    ball = shapes.sphere(1).make_part("ball")
    block = shapes.box(1, 2, 3).make_part("block")
    other_ball = shapes.sphere(1).make_part("ball")      # a distinct Part with the same name
    inner = cc.assembly("inner", [block.translated_x(3), ball.translated_z(4), block.hidden()])
    hidden_inner = cc.assembly("unseen", [ball.translated_y(9)]).hidden()
    return cc.assembly("top", [ball, block.rotated_z(30).translated_y(-2), ball.translated_x(-3).hidden(), inner.translated_z(1),
                               hidden_inner, other_ball.translated_x(6)]), (ball, block, other_ball)


def test_exports():
    for name in ("render_assembly_pixels", "render_assembly_pil_image", "render_assembly_image"):
        assert getattr(rendering, name) is getattr(ap, name)


def test_ids_index_the_visible_instances_in_listing_order():
    asm, (ball, block, other_ball) = _assembly()
    instances, hues, camera, a = ap.scene(asm, (64, 48))
    every = list(asm.all_instances())
    assert len(every) == 8 and [i.visible for i in every] == [True, True, False, True, True, False, False, True]
    assert [i.name for i in instances] == ["ball", "block", "block", "ball", "ball"]
    assert [i.part for i in instances] == [i.part for i in every if i.visible]
    assert [i.transform for i in instances] == [i.transform for i in every if i.visible]
    assert hues.shape == (5, 3) and hues.dtype == numpy.float32
    assert (hues == numpy.float32(ap.DEFAULT_HUE)).all()
    # the assembly's own transform places every instance
    moved = asm.translated_x(5).rotated_y(20)
    placed = ap.scene(moved, (64, 48))[0]
    assert [i.transform for i in placed] == [moved.transform * i.transform for i in every if i.visible]


def test_colors_per_part():
    asm, (ball, block, other_ball) = _assembly()
    instances = ap.scene(asm, (64, 48))[0]
    hues = ap.part_colors(instances, "parts")
    for i, a in enumerate(instances):
        for j, b in enumerate(instances):
            assert (a.part is b.part) == bool((hues[i] == hues[j]).all()), (i, j)
    # BOM order: ball, block, the other ball
    assert [tuple(h) for h in hues[[0, 1, 4]]] == [tuple(numpy.float32(c)) for c in ap.PALETTE[:3]]
    assert len(set(ap.PALETTE)) == len(ap.PALETTE) and ap.PALETTE[0] == ap.DEFAULT_HUE
    given = [(0, 0, 0), (1, 1, 1), (0.5, 0.25, 0.125), (1, 0, 0), (0, 0, 1)]
    assert ap.part_colors(instances, given).tolist() == [list(c) for c in given]
    named = ap.part_colors(instances, {"block": (1, 0, 0)})
    assert named[[1, 2]].tolist() == [[1, 0, 0]] * 2 and (named[[0, 3, 4]] == numpy.float32(ap.DEFAULT_HUE)).all()
    assert ap.scene(asm, (64, 48), colors={"ball": (0, 1, 0)})[1][[0, 3, 4]].tolist() == [[0, 1, 0]] * 3


@pytest.mark.parametrize("bad", [
    [(1, 0, 0)] * 4, [(1, 0, 0)] * 6, {"nut": (1, 0, 0)}, {"unseen": (1, 0, 0)}, [(1, 0, 0)] * 4 + [(1.5, 0, 0)],
    [(1, 0, 0)] * 4 + [(0, -0.1, 0)], [(1, 0, 0)] * 4 + [(0, float("nan"), 0)], {"ball": (0, 0, 2)}, [(1, 0)] * 5, [1, 2, 3, 4, 5],
    "rainbow", {"ball": "red"}])
def test_bad_colors_are_value_errors_before_any_launch(bad):
    asm, _ = _assembly()
    with pytest.raises(ValueError):
        ap.scene(asm, (64, 48), colors=bad)
    with pytest.raises(ValueError):      # (no device here: a launch would be a RuntimeError)
        ap.render_assembly_pixels(asm, (64, 48), colors=bad)


def test_what_cannot_be_rendered():
    ball = shapes.sphere(1).make_part("ball")
    crowd = cc.assembly("crowd", [ball.translated_x(3 * i) for i in range(65)])
    with pytest.raises(ValueError, match="64"):
        ap.render_assembly_pixels(crowd, (64, 48))
    assert len(ap.scene(cc.assembly("crowd", [ball.translated_x(3 * i) for i in range(64)] + [ball.hidden()]), (64, 48))[0]) == 64
    with pytest.raises(ValueError, match="visible"):
        ap.render_assembly_pixels(cc.assembly("ghosts", [ball.hidden(), ball.translated_x(3).hidden()]), (64, 48))
    with pytest.raises(ValueError, match="3D"):
        ap.render_assembly_pixels(cc.assembly("flat", [shapes.circle(1).make_part("disc")]), (64, 48))
    with pytest.raises(ValueError, match="assembly"):
        ap.render_assembly_pixels(shapes.sphere(1), (64, 48))


@pytest.mark.parametrize("placed", [False, True])
@pytest.mark.parametrize("view_angle", [None, 35])
def test_the_camera_is_the_unions(placed, view_angle):
    asm, _ = _assembly()
    if placed:
        asm = asm.rotated((1, 2, 3), 40).translated(5, -7, 2)
    size = (96, 64)
    instances, hues, camera, a = ap.scene(asm, size, view_angle)
    united = asm.shape()
    want_camera = ray_caster.get_camera_params(united.bounding_box(), size, view_angle)
    want = ray_caster.kernel_arguments(united, *want_camera)
    assert tuple(camera[0]) == tuple(want_camera[0]) and tuple(camera[1]) == tuple(want_camera[1])
    assert tuple(camera[2]) == tuple(want_camera[2]) and camera[3] == want_camera[3]
    assert sorted(a) == sorted(want)
    for key in want:
        got, ref = a[key], want[key]
        assert (tuple(got) == tuple(ref)) if hasattr(ref, "__iter__") else (got == ref), key


def test_part_at():
    asm, _ = _assembly()
    from codecad_amd.interference import Instance
    instances = [Instance(i.name, i) for i in ap.scene(asm, (4, 2))[0]]
    ids = numpy.array([[-1, 0, 1, 4], [2, -1, -1, 3]], dtype=numpy.int32)
    picture = ap.AssemblyPicture(None, ids, None, instances, None, None, None, None)
    assert picture.part_at(0, 0) is None and picture.part_at(3, 0) is instances[4] and picture.part_at(0, 1) is instances[2]
    assert picture.part_at(1, 0).name == "ball" and picture.part_at(2, 0).instance.part.name == "block"


def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in ("hu_ray_caster_instances", "hu_instance_table"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
    with open(_lib.HEADER) as f:
        header = f.read()
    # the table arguments first, in the order the instance entry points take them; then hu_ray_caster's
    proto = re.search(r"int hu_ray_caster_instances\(([^;]*)\);", header).group(1)
    names = [re.split(r"[\s*]+", re.sub(r"\[\d*\]", "", p.strip()))[-1] for p in proto.split(",")]
    assert names[:4] == ["table_dev", "n", "distance_only", "lane_bytes"]
    single = re.search(r"int hu_ray_caster\(([^;]*)\);", header).group(1)
    single_names = [re.split(r"[\s*]+", re.sub(r"\[\d*\]", "", p.strip()))[-1] for p in single.split(",")]
    assert names[4:4 + len(single_names) - 3] == single_names[1:-2]
    assert names[-7:] == ["colors_dev", "out_dev", "part_ids_dev", "depth_dev", "flags", "counters_dev", "stream"]
    assert len(_lib.PROTOTYPES["hu_ray_caster_instances"]) == len(names)
    # argument checks need no device
    v = (ctypes.c_float * 4)(0, 0, 0, 0)
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(table=p, n=2, distance_only=0, lane_bytes=64, options=0, w=8, h=8, colors=p, flags=0):
        return lib.hu_ray_caster_instances(table, n, distance_only, lane_bytes, v, v, v, v, 0.1, 1.0, 0.0, 1.0, 0.0, options, w, h,
                                           colors, p, p, p, flags, None, None)
    for kwargs in ({"table": None}, {"colors": None}, {"n": 0}, {"n": 65}, {"distance_only": 1}, {"lane_bytes": 0}, {"lane_bytes": 20},
                   {"options": 4}, {"w": 0}, {"h": 0}, {"flags": 2}):
        assert call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    dl, lb = ctypes.c_int(0), ctypes.c_uint32(0)
    tapes = (ctypes.c_void_p * 1)(None)
    assert lib.hu_instance_table(tapes, 1, 1, buf, 64, ctypes.byref(dl), ctypes.byref(lb)) == -3
    assert lib.hu_instance_table(tapes, 65, 1, buf, 64, ctypes.byref(dl), ctypes.byref(lb)) == -3


def test_the_kernel_keeps_its_records_in_scalar_registers(tmp_path):
    """What tests/test_assemblies.py asks of the interference and clearance kernels, of k_ray_caster_instances: no scratch
    (clearance's leaf is the model: its per-instance values live in LDS, not in a private array); no vector-memory load at
    all -- arguments, the instance table, the colour table, the records and constants of every program are wave-uniform --;
    and the interpreter's fetch groups as wide scalar loads off a pointer that was itself loaded from memory (an
    instance's program out of the table), not only the wide load of the kernel arguments.  Its stores are ordinary
    vector stores."""
    from codecad_amd.hip_util import builder
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    assert "instance_rays.hip" in builder.SOURCES and "instance_rays.hip" not in builder.FLAGGED_SOURCES
    out = tmp_path / "instance_rays.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_rays.hip")], check=True, capture_output=True)
    text = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\w+)", text)
    assert len(kernels) == 1 and "k_ray_caster_instances" in kernels[0]
    assert re.search(r"\.private_segment_fixed_size:\s*0\b", text.split(".amdgpu_metadata")[1])
    chunk = [c for c in re.split(r"\n(?=_Z\w+:\s+; @)", text) if c.startswith(kernels[0] + ":")][0]
    scratch = re.search(r"; ScratchSize: (\d+)", chunk)
    assert scratch and int(scratch.group(1)) == 0
    body = chunk.split(".section")[0]
    assert not re.search(r"\t(flat|global|buffer|scratch)_load", body)
    assert not re.search(r"\tscratch_", body)
    loaded = set(re.findall(r"\ts_load_dwordx[24] s\[(\d+):\d+\]", body))       # pointers read from memory
    wide = collections.Counter(re.findall(r"\ts_load_dwordx(?:8|16) s\[\d+:\d+\], s\[(\d+):\d+\]", body))
    assert any(n >= 2 and base in loaded for base, n in wide.items())
    stores = set(re.findall(r"\t((?:flat|global|buffer)_(?:store|atomic)\w*)", body))
    assert stores and all(s.startswith("global_") for s in stores), stores
