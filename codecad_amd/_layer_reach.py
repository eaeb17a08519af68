"""What `drainage()` and `islands()` do alike on the device (csrc/instance_reach.hip): monotone reachability over the part-id
volume, connected within a layer and handed on from layer to layer in one direction only.  A caller labels the layers'
components of its set (`hu_drain_layers`, `hu_ground_layers`); `hu_components_flatten` makes every entry its root; the caller
seeds, setting bit 31 of a root's entry; `hu_drain_rise` is one PASS up every line of the axis that hands the flags on from a
layer to the next, repeated until a pass sets no flag.  Between the launches the host waits only for the word of a pass."""
import numpy

from . import hip_util
from .hip_util import check


def rise(manager, layers_ptr, word, dims, pz, axis, up):
    """Passes of `hu_drain_rise` over the flattened, seeded labels at `layers_ptr` until one leaves the Buffer `word` zero ->
    how many ran: at most n_axis + 1, a chain of handovers climbs a layer a link.  `manager`: the caller's `hip_manager`."""
    lib, queue = manager.lib, manager.queue
    passes = 0
    while True:
        check(lib.hu_memset(word.device_ptr, 0, word.size, queue.handle), "hu_memset")
        check(lib.hu_drain_rise(layers_ptr, word.device_ptr, dims, pz, axis, int(up), queue.handle), "hu_drain_rise")
        passes += 1
        if int(word.read()[0]) == 0:
            return passes


def flagged_layers(manager, volume, dims, axis, up, counters, label, seed):
    """The zeroed uint64 counters of shape `counters`, the word and the labels of the ids in the Buffer `volume`, flags final
    -> (acc, word, layers, passes).  `label(acc, layers)` and `seed(acc, layers)` enqueue the caller's stage 1 and stage 2;
    `manager` is the caller's `hip_manager`: the library and the queue are those the caller launches its own stages on."""
    lib, queue = manager.lib, manager.queue
    pz = volume.shape[2]
    acc = hip_util.Buffer(numpy.uint64, counters, queue=queue)
    check(lib.hu_memset(acc.device_ptr, 0, acc.size, queue.handle), "hu_memset")
    word = hip_util.Buffer(numpy.uint32, (1,), queue=queue)
    layers = hip_util.Buffer(numpy.uint32, volume.shape, queue=queue)
    label(acc, layers)
    check(lib.hu_components_flatten(layers.device_ptr, dims, pz, queue.handle), "hu_components_flatten")
    seed(acc, layers)
    return acc, word, layers, rise(manager, layers.device_ptr, word, dims, pz, axis, up)


def box_layers(box, na, axis, up):
    """(lowest, highest) layer of the index box ((x0, y0, z0), (x1, y1, z1)) along `axis` of `na` samples."""
    lo, hi = box[0][axis], box[1][axis]
    return (lo, hi) if up else (na - 1 - hi, na - 1 - lo)
