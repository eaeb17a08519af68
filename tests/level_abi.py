"""The launch record of a level of a tape's hierarchy (include/hip_util.h hu_level_launch), filled for the host tests of the
argument checks of hu_subdivision_level and hu_mass_properties_level: every pointer is FAKE and max_parents and capacity are 0,
so that not even a check that let something through could launch a kernel over the made-up pointers.  A test breaks one field
by naming it; ctypes passes a record by reference where a prototype takes a pointer to one, and None as NULL."""
from codecad_amd.hip_util._lib import LevelLaunch

FAKE = 4096                     # never dereferenced: each call is rejected first
NULL_RECORD = {"record": None}  # launch(**NULL_RECORD) is NULL


def launch(**overrides):
    """A record both entry points accepts: an empty list of parents of 8^3 cells, no room for children, every cell kept."""
    fields = dict(tape=FAKE, parents_dev=FAKE, n_parents_dev=FAKE, counter_dev=FAKE, children_dev=FAKE, stream=None, max_parents=0,
                  capacity=0, world=1, rank=0, dims=(8, 8, 8), step=0.1, thr=0.1)
    fields.update(overrides)
    return None if "record" in fields else LevelLaunch(**fields)
