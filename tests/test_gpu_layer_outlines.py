"""layer_outlines() on the device against the reference stack of layer_outlines_scenes.py (the oracle at the ringed samples
of every layer, crossings in NumPy float32, segments derived from the crossed edges, the layered restatement of the keep
rule) and against section_outlines() on the device, layer by layer.  Every comparison is exact: the sorted records byte for
byte, `counts`, `layer_counts` and the evaluations as integers."""
import xml.etree.ElementTree

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import rendering
from codecad_amd.section import Plane
from codecad_amd.section_outlines import SEGMENT, Outlines
from codecad_amd.layer_outlines import LAYER_SEGMENT, Layers, unpack
from codecad_amd.rendering import assembly_section_svg

import layer_outlines_scenes as scenes
import test_section_outlines_host as tso

pytestmark = pytest.mark.gpu


def check(got, ref, evaluations=None):
    assert isinstance(got, Layers) and got.dims == tuple(int(d) for d in ref.dims) and got.step == ref.step
    assert got.heights.tolist() == ref.heights.tolist() and got.corners.tobytes() == ref.corners.tobytes()
    assert all(a.origin.tobytes() == b.origin.tobytes() for a, b in zip(got.planes, ref.planes)) and len(got.planes) == len(ref.planes)
    assert got.segments.dtype == LAYER_SEGMENT and got.segments.tobytes() == ref.segments.tobytes()
    assert got.counts.tolist() == ref.counts.tolist() and got.layer_counts.tolist() == ref.layer_counts.tolist()
    assert [i.instance.transform for i in got.instances] == [i.transform for i in ref.instances]
    if evaluations is not None:
        assert got.evaluations == evaluations


def run(name, cull=True, **kwargs):
    asm, plane, resolution, heights, ref = scenes.scenario(name)
    got = cc.layer_outlines(asm, plane, resolution, heights, cull=cull, **kwargs)
    check(got, ref, scenes.traversal(name, cull).evaluations)
    return got, ref


def test_two_boxes_with_layers_that_miss_and_a_layer_a_step_below_two_faces(hip):
    got, ref = run("two_boxes")
    assert got.runs == 1 and got.layer_counts[0].tolist() == got.layer_counts[5].tolist() == [0, 0]
    assert (got.layer_counts[2:5] > 0).all() and got.layer_counts[1, 0] == 0 < got.layer_counts[1, 1]
    areas = got.areas()
    cut = 4 * 0.0625 ** 2 / 8               # (the four cut corners: test_layer_outlines_host.py)
    assert areas[:, 0].tolist() == pytest.approx([0, 0, 4 - cut, 4 - cut, 4 - cut, 0]) and areas[:, 1].tolist() == pytest.approx([0] + [2 - cut] * 4 + [0])
    layer = got.layer(4)
    assert isinstance(layer, Outlines) and layer.points3d(layer.loops[0][0])[:, 2].tolist() == [0.9375] * len(layer.loops[0][0].points)


def test_boxes_and_ball_on_an_oblique_plane(hip):
    got, ref = run("boxes_and_ball")
    assert got.runs == 1 and len(got.heights) == 5 and (got.layer_counts.sum(axis=1) > 0).all()


def test_both_saddles_on_every_layer(hip):
    got, ref = run("diagonal")
    for l in range(3):
        loops = got.layer(l).loops[0]
        assert len(loops) == 3 and all(loop.closed and loop.area > 0 for loop in loops)


def test_a_tile_with_a_single_live_column(hip):
    got, ref = run("bar_64_9")
    assert got.dims == (64, 9) and got.segments["a"].max() == 64 and (got.layer_counts[:, 0] > 0).all()


def test_64_instances_without_the_hidden_ones(hip):
    got, ref = run("grid_64")
    k = unpack(got.segments["word"])[0]
    assert len(got.instances) == 64 and k.min() < 32 <= k.max() and (got.counts > 0).sum() > 30


def test_far_from_the_origin(hip):
    run("far")


def test_coincident_instances_give_identical_segments_on_every_layer(hip):
    got, ref = run("coincident")
    k, _, _, layer = unpack(got.segments["word"])
    for l in range(3):
        a, b = got.segments[(layer == l) & (k == 0)].copy(), got.segments[(layer == l) & (k == 1)].copy()
        b["word"] -= 1
        assert len(a) > 0 and a.tobytes() == b.tobytes()


def test_70000_layers_of_one_sample(hip):
    asm, plane, resolution, heights, records, evaluations = scenes.speck_reference()
    got = cc.layer_outlines(asm, plane, resolution, heights)
    assert got.runs == 1 and got.dims == (1, 1) and got.segments.tobytes() == records.tobytes()
    assert got.evaluations == evaluations and got.counts.tolist() == [4 * scenes.SPECK_LAYERS]
    assert got.layer_counts.shape == (scenes.SPECK_LAYERS, 1) and (got.layer_counts == 4).all()
    assert unpack(got.segments["word"])[3].max() == scenes.SPECK_LAYERS - 1 > 65535
    assert len(got.layer(65536).loops[0][0].points) == 4


@pytest.mark.parametrize("name", ["boxes_and_ball", "grid_64"])
def test_dense_gives_what_culled_gives(hip, name):
    dense, culled = run(name, cull=False)[0], run(name)[0]
    assert dense.segments.tobytes() == culled.segments.tobytes() and dense.evaluations > culled.evaluations and dense.runs == 1


def test_overflowing_lists_and_segment_buffers_are_regrown(hip):
    first = run("boxes_and_ball")[0]
    both = run("boxes_and_ball", initial_capacity=1, segment_capacity=1)[0]
    assert first.runs == 1 and both.runs > 1


@pytest.mark.parametrize("name", ["two_boxes", "grid_64"])
def test_the_stack_is_the_loop_on_the_device(hip, name):
    asm, plane, resolution, heights, ref = scenes.scenario(name)
    got = cc.layer_outlines(asm, plane, resolution, heights)
    evaluations = 0
    for l, h in enumerate(heights):
        single = cc.section_outlines(asm, scenes.named_plane(plane, h), resolution)
        layer = got.layer(l)
        assert layer.segments.dtype == SEGMENT and layer.segments.tobytes() == single.segments.tobytes()
        assert layer.corner.tobytes() == single.corner.tobytes() and layer.dims == single.dims
        assert layer.counts.tolist() == single.counts.tolist()
        evaluations += single.evaluations
    assert got.evaluations == evaluations


def test_the_drawings_of_a_stack(hip, tmp_path):
    asm, plane, resolution, heights, ref = scenes.scenario("two_boxes")
    got = rendering.render_assembly_layers_svg(asm, str(tmp_path), plane, resolution, heights)
    check(got, ref)
    for l in range(len(heights)):
        path = tmp_path / ("layer_%05d.svg" % l)
        root = xml.etree.ElementTree.parse(str(path)).getroot()
        layer = got.layer(l)
        assert path.read_text() == assembly_section_svg.assembly_section_svg_document(layer)
        paths = [e for e in root if e.tag.endswith("path")]
        assert len(paths) == sum(1 for loops in layer.loops if loops) and all(p.get("fill-rule") == "evenodd" for p in paths)
        tso.check_raster_property(layer.segments, ref.w[l], float(got.step))       # the even-odd fill of the loops: the inside map
