"""hu_blocking_lines alone on the raw volumes of raw_volume_scenes.py, against disassembly_scenes.reference_blocking (the
definition): 64 random parts with a padding that would make pairs, ids from n up that must count as empty, and volumes so wide
that a wavefront of the walks along x and y takes a second unit, whose parts its first unit never met.
(test_raw_volumes_host.py shows on the CPU that a stale last index would give other keys there.)"""
import ctypes
import sys

import numpy
import pytest

from codecad_amd import hip_util
from codecad_amd.hip_util import check

import raw_volume_scenes as raw
import disassembly_scenes as dis

pytestmark = pytest.mark.gpu
disassembly = sys.modules["codecad_amd.disassembly"]


def blocking(hip, ids, n, axes=(0, 1, 2)):
    """(distance, witness) of the key table after hu_blocking_lines over `axes`, one stream, keys set to all ones."""
    buffer, pz = raw.padded(ids, raw.BLOCK_POISON)
    volume = hip_util.Buffer(numpy.uint8, buffer.shape, queue=hip.queue)
    volume.enqueue_write(buffer)
    keys = hip_util.Buffer(numpy.uint64, disassembly._KEYS, queue=hip.queue)
    keys.enqueue_fill(0xff)
    dims = (ctypes.c_uint32 * 3)(*ids.shape)
    for axis in axes:
        check(hip.lib.hu_blocking_lines(volume.device_ptr, keys.device_ptr, dims, pz, axis, n, hip.queue.handle), "hu_blocking_lines")
    table = keys.read().copy()
    for b in (volume, keys):
        b.release()
    ones = numpy.uint64(disassembly._ONES)
    assert (table[:, n:] == ones).all() and (table[:, :, n:] == ones).all()         # nothing beyond the n parts is touched
    return disassembly._decode(table, n)


def check_tables(got, want):
    for array, ref in zip(got, want):
        for axis in range(3):
            wrong = numpy.argwhere(array[axis] != ref[axis])
            assert len(wrong) == 0, (axis, [(tuple(k), int(array[axis][tuple(k)]), int(ref[axis][tuple(k)])) for k in wrong[:8]])


@pytest.mark.parametrize("n", [64, 40])
def test_64_random_parts_and_ids_from_n_up(hip, n):
    got = blocking(hip, raw.block_small_ids(), n)
    want = raw.block_small_reference(n)
    print("n", n, "finite", int((got[0] != dis.NEVER).sum()), "reference", int((want[0] != dis.NEVER).sum()))
    check_tables(got, want)


@pytest.mark.parametrize("na", raw.WIDE_NA)
@pytest.mark.parametrize("axis", [0, 1])
def test_a_wavefront_walks_a_second_unit(hip, axis, na):
    ids = raw.wide_ids(axis, na)
    want = raw.wide_reference(axis, na)
    got = blocking(hip, ids, raw.WIDE_PARTS)
    print("axis", axis, "na", na, "distance", got[0][axis].tolist(), "reference", want[0][axis].tolist())
    check_tables(got, want)
