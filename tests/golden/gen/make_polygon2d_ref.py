#!/usr/bin/env python3
"""Record the executed reference contouring kernel (oracle/_ref/libref_polygon2d.so, built by oracle/ref_cl.py from
the reference's own rendering/polygon2d.cl) on the synthetic fields of tests/polygon2d_scenes.py
-> tests/golden/polygon2d_ref.npz.

Inputs are not stored: every field is a function of its seed.  Outputs are stored in full per scene:
"<scene>/v" vertices as uint32 bit patterns (cells, 2), unwritten cells 0xffffffff; "<scene>/l" links (cells,);
"<scene>/s" starts in launch order.  The two largest noise grids stay out to keep the file under 256 KB.

    python tests/golden/gen/make_polygon2d_ref.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def record():
    import oracle
    import polygon2d_scenes as ps
    out = {}
    for s in ps.fixture_scenes() + ps.on_constant_scenes():
        v, l, st = oracle.ref_process_polygon(s.corners, s.corner, s.step)
        out[s.name + "/v"] = v.view(np.uint32)
        out[s.name + "/l"] = l
        out[s.name + "/s"] = st
    return out


if __name__ == "__main__":
    import oracle
    import polygon2d_scenes as ps
    oracle.build()
    np.savez_compressed(ps.FIXTURE, **record())
    size = os.path.getsize(ps.FIXTURE)
    assert size < 256 * 1024, size
    print("wrote %s: %d bytes" % (os.path.relpath(ps.FIXTURE, ROOT), size))
