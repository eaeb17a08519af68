"""Folded chains (csrc/specialise.hpp fold_chains), host only: the source the generator writes for the distance walks over
boxes.  A union of scaled unions reads one pair column per plane instead of one per (plane, level); the float4 walks and
the in-place form keep the tree as it is; nothing folds where box pruning guards an operand."""
import ctypes
import re

import numpy as np

import codecad_amd as cc
from codecad_amd.hip_util import _lib


def _source(shape):
    lib = _lib.load()
    t = np.ascontiguousarray(cc.nodes.make_program(shape), dtype=np.float32)
    p = t.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    needed = ctypes.c_size_t(0)
    assert lib.hu_tape_source(p, t.size, None, 0, ctypes.byref(needed)) == 0
    buf = ctypes.create_string_buffer(needed.value)
    assert lib.hu_tape_source(p, t.size, buf, needed.value, ctypes.byref(needed)) == 0
    return buf.value.decode()


def _body(src, head):
    at = src.index(head)
    return src[at:src.index("\n}\n", at)]


def _columns(src, tag):
    m = re.search(r"// %s: hoisted out of walks along x: \d+ values; table columns: (\d+) / (\d+) / (\d+) \(x / y / z\), "
                  r"(\d+) / (\d+) / (\d+) \(xy / xz / yz\)" % tag, src)
    assert m, tag
    return tuple(int(g) for g in m.groups())


def test_sponge4_distance_walk_reads_one_column_per_plane():
    src = _source(cc.examples.sponge(4))
    # float4 walks: the thirteen pair columns of the four levels and the outer box, as before
    assert _columns(src, "_x")[3:] == (5, 4, 4)
    # distance walks: one folded column per plane, plus the outer box's xy column
    assert _columns(src, "_d")[3:] == (2, 1, 1)
    dist = _body(src, "auto tape_dist_x(")
    assert dist.count("tb.template XY<") == 2 and dist.count("tb.template XZ<") == 1 and "YZ<" not in dist
    assert dist.count("min3_x(") == 1 and "min_x(" not in dist and " * " not in dist     # the scalings live in the tables
    pre = _body(src, "auto tape_pre_d(")
    assert pre.count("tb.template YZ<") == 1                                            # the folded yz column, once per walk
    # each folded column is the minimum over the four levels of (scale * the level's column)
    for table in ("xy", "xz", "yz"):
        body = _body(src, "void tape_tab_d_%s(" % table)
        assert body.count("min_x(") == 3 and body.count("perp_w_x(") == (5 if table == "xy" else 4)
    # the float4 walk and the in-place form keep the tree (their comparisons pick the directions)
    assert _body(src, "auto tape_eval_x(").count("YZ<") == 0 and _body(src, "auto tape_pre_x(").count("YZ<") == 4
    assert _body(src, "auto tape_dist(").count(" * ") >= 4
    assert "kDPairXY = 2, kDPairXZ = 1, kDPairYZ = 1;" in src and "kPairXY = 5, kPairXZ = 4, kPairYZ = 4;" in src


def test_fold_needs_a_chain_worth_folding():
    s = cc.shapes
    # one rectangle per plane: nothing to group, the distance walk reads what it read
    bar = s.box(0.25, 0.25, float("inf"))
    cross = bar + bar.rotated_x(90) + bar.rotated_y(90)
    src = _source(s.box() - cross)
    assert _columns(src, "_d")[3:] == _columns(src, "_x")[3:] == (2, 1, 1)
    # two scaled copies of the cross where box pruning decides between them: no fold
    two = _source(s.box() - (cross.scaled(0.5) + cross.scaled(0.25)))
    assert _columns(two, "_x")[3:] == _columns(two, "_d")[3:] == (3, 2, 2)
    # ... and behind a repetition (nothing to prune): the bars of one plane fold into one column, in a mirrored frame too
    for inner in (cross.scaled(0.25), cross.scaled(0.25).mirrored_x()):
        rep = _source(s.box() - s.unsafe.Repetition(cross.scaled(0.5) + inner, (1.0, 1.0, 1.0)))
        assert _columns(rep, "_x")[3:] == (3, 2, 2) and _columns(rep, "_d")[3:] == (2, 1, 1)


def test_no_fold_across_pruned_operands():
    # an assembly whose parts box pruning decides: its guarded selects keep their operands, and the distance walk its tests
    s = cc.shapes
    parts = [s.box(1, 1, 1).translated(3 * i, 0, 0) + s.box(1, 1, 1).scaled(0.5).translated(3 * i, 2, 0) for i in range(6)]
    src = _source(s.union(parts))
    m = re.search(r"box pruning: (\d+) scopes", src)
    assert m and int(m.group(1)) > 0
    dist = _body(src, "auto tape_dist_x(")
    assert "alive<" in dist
