"""hu_components_local, _merge, _flatten, _stats and _finish by hand, as assembly_components._label_volume runs them, on the raw
volumes of raw_volume_scenes.py against assembly_components_scenes.reference_components: noise of 64 parts, the worst case for
the union-find, on a lattice that is no multiple of the tile on any axis, a padding that would join S under either `solid`,
and a first table of ONE row, so that the statistics run again without assigning slots -- the labels and every field of every
row EQUAL to the reference."""
import ctypes
import sys

import numpy
import pytest

from codecad_amd import hip_util
from codecad_amd.hip_util import check

import raw_volume_scenes as raw
from raw_volume_scenes import NONE

pytestmark = pytest.mark.gpu
components = sys.modules["codecad_amd.assembly_components"]
ROW = components._ROW


def label(hip, ids, solid, local, capacity):
    """(labels uint32[nx][ny][pz], the table's used rows, how often the statistics ran)"""
    buffer, pz = raw.padded(ids, raw.COMP_POISON)
    lib, queue = hip.lib, hip.queue
    volume = hip_util.Buffer(numpy.uint8, buffer.shape, queue=queue)
    volume.enqueue_write(buffer)
    labels = hip_util.Buffer(numpy.uint32, buffer.shape, queue=queue)
    labels.enqueue_fill(0x5a)
    dims = (ctypes.c_uint32 * 3)(*ids.shape)
    check(lib.hu_components_local(volume.device_ptr, labels.device_ptr, dims, pz, solid, local, queue.handle), "hu_components_local")
    check(lib.hu_components_merge(labels.device_ptr, dims, pz, local, queue.handle), "hu_components_merge")
    check(lib.hu_components_flatten(labels.device_ptr, dims, pz, queue.handle), "hu_components_flatten")
    runs, count = 0, None
    while True:
        table = hip_util.Buffer(ROW, (capacity + 1,), queue=queue)                   # row 0: the counter
        table.enqueue_fill(0)
        check(lib.hu_components_stats(volume.device_ptr, labels.device_ptr, dims, pz, solid, int(count is None), table.device_ptr,
                                      table.device_ptr + ROW.itemsize, capacity, queue.handle), "hu_components_stats")
        rows = table.read().copy()
        table.release()
        runs += 1
        assert runs <= 2
        if count is None:
            count = int(rows[:1].view(numpy.uint32)[0])
        if count <= capacity:
            break
        capacity = count
    check(lib.hu_components_finish(labels.device_ptr, dims, pz, queue.handle), "hu_components_finish")
    out = labels.read().copy()
    for b in (volume, labels):
        b.release()
    return out, rows[1:1 + count], runs


@pytest.mark.parametrize("solid", [0, 1])
@pytest.mark.parametrize("local", [0, 1])
@pytest.mark.parametrize("name", list(raw.COMP_VOLUMES))
def test_the_kernels_by_hand_on_noise(hip, name, local, solid):
    ids = raw.comp_ids(name)
    ref = raw.comp_reference(name, solid)
    nz = ids.shape[2]
    labels, rows, runs = label(hip, ids, solid, local, 1)
    print(name, "local" if local else "global", "solid" if solid else "empty", "components", len(rows), "reference", len(ref.components))
    assert runs == 2 and len(ref.components) > 1                                     # the table was regrown: slots were not assigned again
    wrong = numpy.argwhere(labels[:, :, :nz] != ref.labels)
    assert len(wrong) == 0, [(tuple(k), int(labels[tuple(k)]), int(ref.labels[tuple(k)])) for k in wrong[:8]]
    assert (labels[:, :, nz:] == NONE).all()                                         # the padding is in no component
    assert ((labels[:, :, :nz] == NONE) == (ref.labels == NONE)).all()
    got = [(r.label, r.count, r.box, r.index_sums, r.touches_border, r.parts) for r in components._components(rows, (0.0, 0.0, 0.0), 1.0)]
    assert got == [tuple(r) for r in ref.components]
    assert any(63 in r[5] for r in got)                                              # bit 63 of `parts`


@pytest.mark.parametrize("solid", [0, 1])
def test_a_table_that_holds_every_row_at_once_gives_the_same(hip, solid):
    ids = raw.comp_ids("noise")
    ref = raw.comp_reference("noise", solid)
    labels, rows, runs = label(hip, ids, solid, 1, 4096)
    assert runs == 1 and len(rows) == len(ref.components)
    got = [(r.label, r.count, r.box, r.index_sums, r.touches_border, r.parts) for r in components._components(rows, (0.0, 0.0, 0.0), 1.0)]
    assert got == [tuple(r) for r in ref.components]
