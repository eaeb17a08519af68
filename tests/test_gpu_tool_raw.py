"""hu_tool_tops, hu_tool_dilate, hu_tool_erode and hu_tool_rest alone, in order on one stream with no host wait between them, on
the raw volumes of tool_access_scenes.py against its reference 1: noise of 64 parts, planted tops at the edges of a word, every
direction, every `of`, column counts around the tile of the morphology kernels, K = 0, 1, 5 and 32, a K greater than the
lattice, heights past 16 bits and a profile entry of 65535 -- the keys, the tips, the cut with its crowd, the rest ids and all
128 counts EQUAL to the reference, and no byte of any padding, nor any word beside a field, written."""
import ctypes
import math

import numpy
import pytest

from codecad_amd import hip_util
from codecad_amd.hip_util import check

import raw_volume_scenes as raw
import tool_access_scenes as scenes
import wide_volume_scenes as wide
from tool_access_scenes import RAW_NAMES, RAW_BY_NAME, EMPTY

pytestmark = pytest.mark.gpu
SENTINEL = 0xa5
GUARD = 64                      # words of sentinel on either side of every field


def tool_kernels(hip, c):
    """(keys [nu, nv], tips [nu + 2K, nv + 2K], cut words [nu, nv], the rest buffer [nx][ny][pz], uint64[2, 64] counts, the
    guards) of a raw case."""
    buffer, pz = raw.padded(c.ids, scenes.RAW_POISON)
    lib, queue = hip.lib, hip.queue
    K = math.isqrt(c.tool.radius_sq)
    nu, nv = (c.ids.shape[a] for a in range(3) if a != c.axis)
    pu, pv = nu + 2 * K, nv + 2 * K
    volume = hip_util.Buffer(numpy.uint8, buffer.shape, queue=queue)
    volume.enqueue_write(buffer)
    rest = hip_util.Buffer(numpy.uint8, buffer.shape, queue=queue)
    rest.enqueue_fill(SENTINEL)
    sizes = (nu * nv, pu * pv, nu * nv)                                             # the tops, the tips, the cut: guards between
    starts = [GUARD + sum(sizes[:k]) + k * GUARD for k in range(3)]
    fields = hip_util.Buffer(numpy.uint32, (starts[2] + sizes[2] + GUARD,), queue=queue)
    fields.enqueue_fill(SENTINEL)
    tops, tips, cut = (fields.device_ptr + 4 * s for s in starts)
    profile = hip_util.Buffer(numpy.uint16, (c.tool.radius_sq + 1,), queue=queue)
    profile.enqueue_write(numpy.array(c.tool.profile, dtype=numpy.uint16))
    acc = hip_util.Buffer(numpy.uint64, (2, 64), queue=queue)
    acc.enqueue_fill(0)
    dims = (ctypes.c_uint32 * 3)(*c.ids.shape)
    of = raw.code(c.of)
    check(lib.hu_tool_tops(volume.device_ptr, tops, dims, pz, c.axis, int(c.up), of, queue.handle), "hu_tool_tops")
    check(lib.hu_tool_dilate(tops, profile.device_ptr, tips, nu, nv, c.tool.radius_sq, queue.handle), "hu_tool_dilate")
    check(lib.hu_tool_erode(tips, tops, profile.device_ptr, cut, nu, nv, c.tool.radius_sq, queue.handle), "hu_tool_erode")
    check(lib.hu_tool_rest(volume.device_ptr, tops, cut, rest.device_ptr, acc.device_ptr, dims, pz, c.axis, int(c.up), of, queue.handle),
          "hu_tool_rest")
    words, rest_bytes, counts = fields.read().copy(), rest.read().copy(), acc.read().copy()
    for b in (volume, rest, fields, profile, acc):
        b.release()
    got = [words[s:s + n] for s, n in zip(starts, sizes)]
    guards = numpy.concatenate([words[:starts[0]]] + [words[s + n:s + n + GUARD] for s, n in zip(starts, sizes)])
    return got[0].reshape(nu, nv), got[1].reshape(pu, pv), got[2].reshape(nu, nv), rest_bytes, counts, guards


def check_against_reference(got, ref, shape):
    keys, tips, cut, rest, counts, guards = got
    nz = shape[2]
    want_keys = numpy.where(ref.tops > 0, ref.tops * 256 + (255 - ref.top_ids.astype(numpy.int64)), 0)
    for name, array, want in (("keys", keys, want_keys), ("tips", tips, ref.tips), ("cut", cut >> 8, ref.cut), ("crowd", cut & 255, ref.crowd)):
        wrong = numpy.argwhere(array != want)
        assert len(wrong) == 0, (name, [(tuple(k), int(array[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]])
    wrong = numpy.argwhere(rest[:, :, :nz] != ref.rest_ids)
    assert len(wrong) == 0, ("rest", [(tuple(k), int(rest[tuple(k)]), int(ref.rest_ids[tuple(k)])) for k in wrong[:8]])
    assert (rest[:, :, nz:] == SENTINEL).all()                                      # the padding is never written
    assert (guards == SENTINEL * 0x01010101).all()                                  # nor a word beside a field
    assert [int(v) for v in counts[0]] == ref.undercut_counts and [int(v) for v in counts[1]] == ref.tight_counts


@pytest.mark.parametrize("name", RAW_NAMES)
def test_the_four_kernels_on_raw_volumes(hip, name):
    c = RAW_BY_NAME[name]
    ref = scenes.raw_reference(name)
    got = tool_kernels(hip, c)
    print(name, "undercut", int(got[4][0].sum()), "reference", sum(ref.undercut_counts), "tight", int(got[4][1].sum()), "reference",
          sum(ref.tight_counts), "highest cut", int(got[2].max() >> 8), "reference", int(ref.cut.max()))
    check_against_reference(got, ref, c.ids.shape)


@pytest.mark.parametrize("axis,up", scenes.DIRECTIONS)
def test_an_empty_volume_leaves_zeros(hip, axis, up):
    ids = numpy.full((5, 7, 130), EMPTY, dtype=numpy.uint8)
    c = scenes.RawCase("empty", ids, axis, up, scenes.BALL3, scenes.SOLID)
    got = tool_kernels(hip, c)
    check_against_reference(got, scenes.reference_tool_access(ids, axis, up, scenes.BALL3, scenes.SOLID, 64, pockets=False), ids.shape)
    assert not got[0].any() and not got[1].any() and (got[2] == EMPTY).all() and (got[3][:, :, :130] == EMPTY).all() and not got[4].any()


# ---- past the grid's cap: a wavefront takes a second line unit (wide_volume_scenes.py) --------------------------------------------

@pytest.mark.parametrize("na", raw.WIDE_NA)
@pytest.mark.parametrize("axis", [0, 1])
def test_a_wavefront_walks_a_second_line(hip, axis, na):
    """hu_tool_tops and hu_tool_rest along x and y over 10000 line units: the lines a wavefront walks second hold other parts than
    the first, and half of them no sample of S at all -- their key is 0, whatever key the lane held before."""
    ids = wide.tool_ids(axis, na)
    for up in (True, False):
        for of in wide.TOOL_OFS:
            ref = wide.tool_reference(axis, na, up, of)
            got = tool_kernels(hip, scenes.RawCase("wide", ids, axis, up, wide.TOOL, of))
            check_against_reference(got, ref, ids.shape)
            second = ref.tops[wide.line_kinds() == 1]                                # the lines a wavefront walks second
            assert (second == 0).any() and (second > 0).any()
