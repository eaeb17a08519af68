"""hu_overhang_first_layer, hu_overhang_mark and hu_overhang_columns alone, in order on one stream with no host wait between
them, on the raw volumes of raw_volume_scenes.py against overhangs_scenes.reference_overhangs: 64 parts of noise, every
direction, every reach, a padding that would support the layer z = nz - 1 -- the three id volumes, the depth word and all 129
counts EQUAL to the reference, and the padding of every output left as it was."""
import ctypes

import numpy
import pytest

from codecad_amd import hip_util
from codecad_amd.hip_util import check

import raw_volume_scenes as raw
from disassembly_scenes import DIRECTIONS
from raw_volume_scenes import SOLID, EMPTY

pytestmark = pytest.mark.gpu
SENTINEL = 0xa5
PLATE, WORD = 3 * 64, 3 * 64 + 1        # in the accumulators, as codecad_amd/overhangs.py lays them out


def overhang_kernels(hip, ids, axis, up, reach_sq, of):
    """(overhang, support, landing buffers [nx][ny][pz], uint64[4, 64] accumulators)"""
    buffer, pz = raw.padded(ids, raw.OVER_POISON)
    lib, queue = hip.lib, hip.queue
    volume = hip_util.Buffer(numpy.uint8, buffer.shape, queue=queue)
    volume.enqueue_write(buffer)
    outs = [hip_util.Buffer(numpy.uint8, buffer.shape, queue=queue) for _ in range(3)]
    for b in outs:
        b.enqueue_fill(SENTINEL)
    over, support, landing = outs
    acc = hip_util.Buffer(numpy.uint64, (4, 64), queue=queue)
    acc.enqueue_fill(0)
    word = acc.device_ptr + 8 * WORD
    dims = (ctypes.c_uint32 * 3)(*ids.shape)
    check(lib.hu_overhang_first_layer(volume.device_ptr, word, dims, pz, axis, int(up), raw.code(of), queue.handle), "hu_overhang_first_layer")
    check(lib.hu_overhang_mark(volume.device_ptr, over.device_ptr, word, acc.device_ptr, dims, pz, axis, int(up), reach_sq, raw.code(of),
                               queue.handle), "hu_overhang_mark")
    check(lib.hu_overhang_columns(volume.device_ptr, over.device_ptr, support.device_ptr, landing.device_ptr, word,
                                  acc.device_ptr + 8 * 64, dims, pz, axis, int(up), raw.code(of), queue.handle), "hu_overhang_columns")
    got = [b.read().copy() for b in outs] + [acc.read().copy()]
    for b in outs + [volume, acc]:
        b.release()
    return got


def check_against_reference(got, ref, shape, axis):
    over, support, landing, acc = got
    nz = shape[2]
    for name, array, want in (("overhang", over, ref.overhang_ids), ("support", support, ref.support_ids), ("landing", landing, ref.landing_ids)):
        wrong = numpy.argwhere(array[:, :, :nz] != want)
        assert len(wrong) == 0, (name, [(tuple(k), int(array[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]])
    assert (support[:, :, nz:] == SENTINEL).all() and (landing[:, :, nz:] == SENTINEL).all()     # the padding is never written
    flat = acc.ravel()
    assert int(flat[WORD]) == shape[axis] - ref.first_layer                          # the depth word: 0 for an empty S
    assert [int(v) for v in acc[0]] == ref.overhang_counts
    assert [int(v) for v in acc[1]] == ref.support_counts and [int(v) for v in acc[2]] == ref.landing_counts
    assert int(flat[PLATE]) == ref.plate_landings and (flat[WORD + 1:] == 0).all()


@pytest.mark.parametrize("of", raw.OVER_OFS, ids=str)
@pytest.mark.parametrize("reach_sq", raw.OVER_REACH)
@pytest.mark.parametrize("axis,up", DIRECTIONS)
@pytest.mark.parametrize("name", ["noise", "line64"])
def test_the_three_kernels_on_noise(hip, name, axis, up, reach_sq, of):
    ids = raw.over_ids(name)
    ref = raw.over_reference(name, axis, up, reach_sq, of)
    got = overhang_kernels(hip, ids, axis, up, reach_sq, of)
    print(name, axis, up, reach_sq, of, "overhangs", int(got[3][0].sum()), "reference", sum(ref.overhang_counts), "supports",
          int(got[3][1].sum()), "reference", sum(ref.support_counts), "first layer", ref.first_layer)
    check_against_reference(got, ref, ids.shape, axis)


@pytest.mark.parametrize("axis,up", DIRECTIONS)
def test_an_empty_volume_leaves_the_word_at_zero(hip, axis, up):
    ids = raw.over_ids("empty")
    got = overhang_kernels(hip, ids, axis, up, 8, SOLID)
    check_against_reference(got, raw.over_reference("empty", axis, up, 8, SOLID), ids.shape, axis)
    assert (got[3] == 0).all() and all((a[:, :, :ids.shape[2]] == EMPTY).all() for a in got[:3])
