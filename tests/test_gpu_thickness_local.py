"""hu_thickness_local alone on the raw volumes of wall_thickness_scenes.py, against the rule written offset by offset
(wall_thickness_scenes.raw_local): fields that are no distance transforms, single lines and samples, dims around the tile's
edges and around 64, a ball across a tile corner, every kernel of the entry point (K = 0 .. 32, a halo wider than a tile side,
a lattice narrower than K), the shrunken radius and the tile that is all cap -- every output EQUAL to the reference with the
LDS staging and without it, the keys and the counts too.  The padding of the inputs and their entries outside S are POISONED
(a kernel that reads them as data fails), and the padding of the output still holds its sentinel.
(test_wall_thickness_host.py shows on the CPU that the cases hold these edges.)"""
import ctypes

import numpy
import pytest

from codecad_amd import hip_util
from codecad_amd.hip_util import check

import raw_volume_scenes as raw
import wall_thickness_scenes as scenes

pytestmark = pytest.mark.gpu
SENTINEL = 0xa5
SENTINEL16 = 0xa5a5


def upload(hip, host):
    b = hip_util.Buffer(host.dtype, host.shape, queue=hip.queue)
    b.enqueue_write(host)
    return b


def filled(hip, dtype, shape, byte):
    b = hip_util.Buffer(dtype, shape, queue=hip.queue)
    b.enqueue_fill(byte)
    return b


def local(hip, case, lds, r2=None):
    """hu_thickness_local over the poisoned buffers of `case` -> (the whole output buffer, keys, counts)."""
    ids, field, pz = scenes.raw_buffers(case)
    buffers = [upload(hip, field), upload(hip, ids), filled(hip, numpy.uint16, field.shape, SENTINEL),
               filled(hip, numpy.uint64, (64,), 0xff), filled(hip, numpy.uint64, (64,), 0)]
    dims = (ctypes.c_uint32 * 3)(*case.ids.shape)
    check(hip.lib.hu_thickness_local(buffers[0].device_ptr, buffers[1].device_ptr, buffers[2].device_ptr, buffers[3].device_ptr,
                                     buffers[4].device_ptr, dims, pz, raw.code(case.of), case.r2 if r2 is None else r2, lds,
                                     hip.queue.handle), "hu_thickness_local")
    got = [b.read().copy() for b in buffers[2:]]
    for b in buffers:
        b.release()
    return got


def check_case(got, name):
    out, keys, counts = got
    want, want_keys, want_counts = scenes.raw_reference(name)
    nz = want.shape[2]
    wrong = numpy.argwhere(out[:, :, :nz].astype(numpy.int64) != want)
    assert len(wrong) == 0, [(tuple(k), int(out[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]]
    assert (out[:, :, nz:] == SENTINEL16).all()                                      # the padding of out is not written
    assert [hex(int(k)) for k in keys] == [hex(int(k)) for k in want_keys]
    assert [int(c) for c in counts] == want_counts


@pytest.mark.parametrize("name", scenes.RAW_NAMES)
def test_the_entry_point_alone_equals_the_rule_with_and_without_lds(hip, name):
    case = scenes.RAW_BY_NAME[name]
    got = [local(hip, case, lds) for lds in (1, 0)]
    want = scenes.raw_reference(name)
    print(name, case.ids.shape, "r2", case.r2, "of", case.of, "nonzero", int((want[0] > 0).sum()), "capped", sum(want[2]),
          "device", int((got[0][0][:, :, :case.ids.shape[2]] > 0).sum()), int(got[0][2].sum()))
    for arm in got:
        check_case(arm, name)
    assert got[0][0].tobytes() == got[1][0].tobytes()


def test_a_small_greatest_value_costs_its_own_radius_and_gives_the_same_bytes(hip):
    """The field's greatest value is 10: under every R2 from 9 up the output and the keys are the bytes of R2 = 9."""
    outs = {name: local(hip, scenes.RAW_BY_NAME[name], 1) for name in scenes.LOW_NAMES}
    base = outs["low_r9"]
    for name, (out, keys, counts) in outs.items():
        assert out.tobytes() == base[0].tobytes() and keys.tobytes() == base[1].tobytes(), name
        assert (counts == 0).all() == (name != "low_r9")                             # only R2 = 9 has its cap at 10
