"""The launch records of the entry points over instance cells (include/hip_util.h hu_cells_launch, hu_cells_children), filled
for the host tests of their argument checks: every pointer is FAKE and max_parents is 0, so that not even a check that let
something through could launch a kernel over the made-up pointers.  A test breaks one field by naming it; ctypes passes a
record by reference where a prototype takes a pointer to one, and None as NULL."""
from codecad_amd.hip_util._lib import CellsLaunch, CellsChildren

FAKE = 4096                     # never dereferenced: each call is rejected first
# launch(**NULL_RECORD) and children(**NULL_RECORD) are NULL.  dims and corner are arrays inside the launch record, so the
# cases that passed a NULL dims or a NULL corner became this one.
NULL_RECORD = {"record": None}


def launch(**overrides):
    """A record every entry point accepts: two instances with distance-only programs, a lattice of 8^3, an empty list."""
    fields = dict(table_dev=FAKE, windows_dev=FAKE, parents_dev=FAKE, n_parents_dev=FAKE, evaluations_dev=FAKE, stream=None,
                  n=2, lane_bytes=64, max_parents=0, distance_only=1, dims=(8, 8, 8), corner=(0.0, 0.0, 0.0), step=0.1)
    fields.update(overrides)
    return None if "record" in fields else CellsLaunch(**fields)


def children(**overrides):
    """A children's list every level accepts once its `child_side` is named: no room, a threshold of 0.5."""
    fields = dict(counter_dev=FAKE, children_dev=FAKE, capacity=0, child_side=4, thr=0.5)
    fields.update(overrides)
    return None if "record" in fields else CellsChildren(**fields)


def held(p, dims):
    """launch()'s fields over the real buffer `p` with a list of one row: a NULL parents_dev is then a bad argument too."""
    return dict(table_dev=p, windows_dev=p, parents_dev=p, n_parents_dev=p, evaluations_dev=p, max_parents=1, dims=dims)
