"""The kernels of csrc/instance_reach.hip, for test_drainage_host.py and test_islands_host.py: the unit compiled to assembly
for gfx950 and every kernel's VGPRs, LDS and private segment read from its metadata; and what DESIGN.md states of them."""
import functools
import os
import re
import subprocess
import tempfile

from codecad_amd.hip_util import builder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "instance_reach.hip"
SHARED = ("k_reach_local<true>", "k_reach_local<false>", "k_reach_merge_faces", "k_reach_merge_all", "k_reach_rise<false>",
          "k_reach_rise<true>")
DRAIN = SHARED + ("k_drain_seed", "k_drain_floor<false>", "k_drain_floor<true>")
GROUND = ("k_ground_seed", "k_ground_mark<false>", "k_ground_mark<true>")


def sources():
    """{file name: text} of every source and header under csrc/."""
    found = {}
    for name in sorted(os.listdir(builder.CSRC)):
        if name.endswith((".hip", ".hpp", ".h")):
            with open(os.path.join(builder.CSRC, name)) as f:
                found[name] = f.read()
    return found


def documented_resources(names):
    """{kernel: (VGPRs, LDS bytes)} of `names` as DESIGN.md states them."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    found = {}
    for name in names:
        m = re.search(r"`%s` (\d+) VGPRs and (\d+) B of LDS" % re.escape(name), text)
        assert m, "DESIGN.md states the VGPRs and the LDS of " + name
        found[name] = (int(m.group(1)), int(m.group(2)))
    return found


@functools.lru_cache(maxsize=None)
def compiled_resources():
    """{kernel: (VGPRs, LDS bytes, private segment bytes)} of every kernel of the unit, None without hipcc.  Compiled once."""
    hipcc = builder.find_hipcc()
    if hipcc is None:
        return None
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "instance_reach.s")
        subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", out, os.path.join(builder.CSRC, UNIT)],
                       check=True, capture_output=True)
        with open(out) as f:
            metadata = f.read().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"\d+(k_\w+?)(?:ILb([01])EEEv|E)NS_9ReachArgsE", name)
        assert m, name
        kernel = m.group(1) + ("" if m.group(2) is None else "<%s>" % ("false", "true")[int(m.group(2))])
        found[kernel] = tuple(int(re.search(r"\.%s:\s*(\d+)" % field, block).group(1))
                              for field in ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size"))
    return found
